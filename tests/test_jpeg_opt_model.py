"""The JPEG result at any (quality, sampling) without a GPU: the generalised model (tests/jpeg_opt_model.py) against libjpeg-turbo's own
file (Pillow) byte for byte, its (85, 0) instance against tests/jpeg_model.py, the worst-case bound per setting, csrc/jpeg_tables.hpp
against the model (a stand-alone program under the address and undefined-behaviour sanitizers), and the C ABI: the new symbols, the
two ire_config fields and the struct size of a caller built before them."""
import base64
import ctypes
import io
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as cases      # noqa: E402
import jpeg_model as base       # noqa: E402
import jpeg_opt_model as model  # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES, SAMPLINGS = model.QUALITIES, model.SAMPLINGS
# h x w.  (48, 203): several intervals with a short last one at either sampling (4:4:4: 6 x 26 = 156 MCUs, 9 full intervals and 12;
# 4:2:0: 3 x 13 = 39 MCUs, 4 full intervals and 7).  It and the last two complete the combinations of h mod 16 and w mod 16.
SHAPES = [(1, 1), (8, 8), (9, 9), (16, 16), (17, 16), (16, 17), (24, 40), (45, 37), (33, 129), (48, 203), (27, 32), (20, 29)]
SIZES = [(1, 1), (5, 7), (64, 64), (750, 1000), (1024, 1024), (8192, 8192), (8192, 1), (1, 8192)]


def image(h, w):
    return (cases.noise if (h + w) % 2 else cases.smooth)(h, w, 100 * h + w)


def pillow_file(px, quality, sampling):
    """libjpeg-turbo through Pillow with the model's settings"""
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=quality, subsampling=sampling, optimize=False, restart_marker_blocks=model.R_OF[sampling])
    return bio.getvalue()


def _kind(v):
    return 0 if v % 16 == 0 else 1 if v % 16 <= 8 else 2


def test_the_shapes_reach_every_edge_case():
    """h mod 16 and w mod 16 each in {0}, 1..8 (a dummy Y block row / column at 4:2:0), 9..15 (replication only): all nine pairs"""
    assert {(_kind(h), _kind(w)) for h, w in SHAPES} == set(itertools.product(range(3), repeat=2))
    for s in SAMPLINGS:
        p, r = (16 if s == 2 else 8), model.R_OF[s]
        nmcu = ((48 + p - 1) // p) * ((203 + p - 1) // p)
        assert nmcu // r >= 4 and 0 < nmcu % r < r


def test_model_equals_libjpeg_turbo():
    """Byte equality with Pillow's file for quality=q, subsampling=s, optimize=False, restart_marker_blocks=R on every shape.  49, 50
    and 51 straddle the scaling formula's switch; 1 and 100 hit the clamps of the table entries."""
    for h, w in SHAPES:
        px = image(h, w)
        for q in QUALITIES:
            for s in SAMPLINGS:
                f, p = model.jpeg_file(px, q, s), pillow_file(px, q, s)
                first = next((i for i, (a, b) in enumerate(zip(f, p)) if a != b), None)
                assert f == p, (h, w, q, s, len(f), len(p), first)


def test_the_default_is_the_first_model():
    for name, px in cases.all_cases().items():
        assert model.jpeg_file(px) == model.jpeg_file(px, 85, 0) == base.jpeg_file(px), name
    assert model.HEADER_BYTES == base.HEADER_BYTES == len(model.header(7, 9, 1, 2)) == len(model.header(8192, 8192, 100, 0))
    assert model.R_OF[0] == base.R and [model.size_max(t, 85) for t in (0, 1)] == [base.size_max(t) for t in (0, 1)]
    assert model.mcu_bits_max(85, 0) == base.MCU_BITS_MAX
    for h, w in SIZES:
        assert model.file_bound(h, w, 85, 0) == base.file_bound(h, w) and model.base64_bound(h, w, 85, 0) == base.base64_bound(h, w)


def _argmax_block(table, quality):
    """A coefficient block (zig-zag, the DC as a difference from 0) that takes model.block_bits_max bits: the same dynamic programme
    with back pointers, restated."""
    smax = model.size_max(table, quality)
    dc, ac = base.DC_CODES[table], base.AC_CODES[table]
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


def test_bound():
    lib = _lib.load()
    assert model.mcu_bits_max(100, 0) == 4474 and model.mcu_bits_max(100, 2) == 9448 and model.mcu_bits_max(85, 2) == 5034
    # the bound does not fall as the quality rises (quality 100 sizes the device's buffers): here over the tested qualities, over all
    # hundred in tests/native/jpeg_opt_tables_dump.cpp
    for s in SAMPLINGS:
        bits = [model.mcu_bits_max(q, s) for q in QUALITIES]
        assert bits == sorted(bits)
    for q in QUALITIES:
        for table in (0, 1):                  # every category has a code; the bound is reached by a real symbol sequence, and by nothing longer
            smax = model.size_max(table, q)
            assert smax[0] <= 11 and max(smax[1:]) <= 10
            zz = _argmax_block(table, q)
            assert sum(l for _, l in base.block_symbols(zz, 0, table)) == model.block_bits_max(table, q)
            rng = np.random.default_rng(1000 * q + table)
            for _ in range(40):
                mag = rng.integers(0, 1 << np.array(smax)) * (rng.random(64) < rng.random())
                assert sum(l for _, l in base.block_symbols((mag * rng.choice([-1, 1], 64)).tolist(), 0, table)) <= model.block_bits_max(table, q)
    # the exact terms of islow behind the categories at quality 100: the DC and the three AC terms with both frequencies in {0, 4}
    y, x = np.mgrid[:8, :8]
    for u, v in ((0, 0), (0, 4), (4, 0), (4, 4)):
        basis = np.cos((2 * y + 1) * u * np.pi / 16) * np.cos((2 * x + 1) * v * np.pi / 16)
        worst = max(abs(int(base.fdct_islow(np.where(sign * basis >= 0, 127, -128)[None])[0, u, v])) for sign in (1, -1))
        assert worst == (model.DC_MIN if (u, v) == (0, 0) else model.EXACT_AC_MAX), (u, v, worst)
    # the worst cases of the first bound test at every quality and both samplings; full-scale noise too at quality 100
    images = cases.all_cases()
    worst = ["checker1", "checker1_inv", "checker8", "checker4", "impulses", "saturated", "wrap24x136", "7x5", "mod3_1"]
    for q in QUALITIES:
        smax = [model.size_max(t, q) for t in (0, 1)]
        for s in SAMPLINGS:
            for name in worst + (["noise160"] if q == 100 else []):
                px = images[name]
                h, w, _ = px.shape
                f = model.jpeg_file(px, q, s)
                assert len(f) <= model.file_bound(h, w, q, s), (name, q, s)
                assert lib.ire_jpeg_base64_bound_ex(h, w, q, s) == model.base64_bound(h, w, q, s) >= len(base64.b64encode(f)), (name, q, s)
                for m in model.mcus(px, q, s):
                    for table, zz in m:
                        assert all(int(abs(v)).bit_length() <= smax[table][p] for p, v in enumerate(zz)), (name, q, s)
    # the checkerboard of period 8 swings the DC over its whole range, and at quality 100 that is the largest category there is
    dcs = [int(m[0][1][0]) for m in model.mcus(images["checker8"], 100, 0)]
    assert (max(dcs) - min(dcs)).bit_length() == model.size_max(0, 100)[0] == 11
    for h, w in SIZES:
        for q, s in ((1, 0), (60, 2), (100, 2), (100, 0)):
            assert lib.ire_jpeg_base64_bound_ex(h, w, q, s) == model.base64_bound(h, w, q, s) > 0
        assert lib.ire_jpeg_base64_bound_ex(h, w, 0, 0) == lib.ire_jpeg_base64_bound(h, w) == base.base64_bound(h, w)      # 0: quality 85
    for h, w, q, s in ((0, 8, 85, 0), (8, 8193, 85, 2), (8, 8, 101, 0), (8, 8, -1, 0), (8, 8, 85, 1), (8, 8, 85, 3), (8, 8, 85, -2)):
        assert lib.ire_jpeg_base64_bound_ex(h, w, q, s) == 0 == model.base64_bound(h, w, q, s), (h, w, q, s)


def test_tables_header_against_the_model(tmp_path):
    """csrc/jpeg_tables.hpp's (quality, sampling) forms, compiled alone with -fsanitize=address,undefined: tables, heads and bounds are
    the model's; the reciprocal identity holds for every divisor 8 q, q in 1..255, and every x < 2^16."""
    exe = str(tmp_path / "jpeg_opt_tables_dump")
    src = os.path.join(ROOT, "tests", "native", "jpeg_opt_tables_dump.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    hws = [(1, 1), (5, 7), (45, 37), (1024, 1024), (8192, 8192), (8192, 1), (1, 8192)]
    args = ["q"] + [str(q) for q in QUALITIES] + ["s"] + [str(s) for s in SAMPLINGS] + ["hw"] + [str(v) for hw in hws for v in hw]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())

    def ints(key):
        return [int(v) for v in got[key].split()]

    assert ints("header_bytes") == [model.HEADER_BYTES] and ints("R") == [model.R_OF[0], model.R_OF[2]]
    for q in QUALITIES:
        for t, tab in enumerate(model.quant_tables(q)):
            assert ints("quant%d q%d" % (t, q)) == tab and ints("size_max%d q%d" % (t, q)) == model.size_max(t, q)
            assert ints("block_bits_max%d q%d" % (t, q)) == [model.block_bits_max(t, q)]
        for s in SAMPLINGS:
            assert ints("mcu_bits_max q%d s%d" % (q, s)) == [model.mcu_bits_max(q, s)]
            assert ints("interval_bound q%d s%d" % (q, s)) == [model.interval_bound(1, q, s), model.interval_bound(model.R_OF[s], q, s)]
            for h, w in hws:
                assert bytes.fromhex(got["header %d %d q%d s%d" % (h, w, q, s)]) == model.header(h, w, q, s)
                assert ints("bound %d %d q%d s%d" % (h, w, q, s)) == [model.file_bound(h, w, q, s), model.base64_bound(h, w, q, s)]
    assert ints("default_is_85_0") == [1]
    assert ints("recip_checked") == [255 * 65536]
    assert ints("largest_sizes") == [11, 10] and ints("bound_monotone") == [1]


def test_abi_symbols_and_config():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ire_jpeg_base64_bound_ex", "ire_encode_jpeg_base64_fit_device_ex", "ire_encode_jpeg_base64_fit_ex"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert [n for n, _ in _lib.IreConfig._fields_][-2:] == ["jpeg_quality", "jpeg_sampling"]
    assert ctypes.sizeof(_lib.IreConfig) == 48 and _lib.IreConfig.jpeg_quality.offset == 36 and _lib.IRE_ABI_VERSION == lib.ire_abi_version() == 3
    import torch
    accepted = _lib.IRE_OK if torch.cuda.is_available() else _lib.IRE_ERR_UNAVAILABLE      # as far as the device check

    def init(size, flags, quality, sampling):
        h = ctypes.c_void_p()
        cfg = _lib.IreConfig()
        cfg.struct_size, cfg.max_batch, cfg.flags, cfg.jpeg_quality, cfg.jpeg_sampling = size, 2, flags, quality, sampling
        st = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
        err = lib.ire_last_error()
        if st == _lib.IRE_OK:
            lib.ire_shutdown(h)
        return st, err

    full, old = ctypes.sizeof(_lib.IreConfig), 40
    for q, s in ((0, 0), (1, 0), (100, 2), (60, 2), (0, 2), (75, 0)):
        assert init(full, _lib.IRE_FLAG_RESULT_JPEG, q, s)[0] == accepted, (q, s)
    for q, s in ((101, 0), (-1, 0), (85, 1), (85, 3), (85, -1), (1000, 2)):            # out of range; 4:2:2 and grey are not built
        st, err = init(full, _lib.IRE_FLAG_RESULT_JPEG, q, s)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"invalid" in err and b"JPEG" in err, (q, s, err)
    for flags in (0, _lib.IRE_FLAG_RESULT_PNG_BASE64, _lib.IRE_FLAG_RESULT_PNG_DEFLATE, _lib.IRE_FLAG_DECODE_PROGRESSIVE):      # settings without the JPEG flag
        for q, s in ((60, 0), (0, 2), (60, 2)):
            st, err = init(full, flags, q, s)
            assert st == _lib.IRE_ERR_INVALID_INPUT and b"IRE_FLAG_RESULT_JPEG" in err, (flags, q, s, err)
        assert init(full, flags, 0, 0)[0] == accepted
    # a caller built before the two fields passes the old size: accepted, and what lies behind its struct is not read
    for flags in (0, _lib.IRE_FLAG_RESULT_JPEG):
        assert init(old, flags, 12345, -7)[0] == accepted, flags
    for size in (0, 4, old - 1):
        st, err = init(size, 0, 0, 0)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"struct_size" in err, size
    assert init(old + 4, _lib.IRE_FLAG_RESULT_JPEG, 12345, 0)[0] == accepted           # (the size covers one field only: neither is read)
    # null handles are rejected, not dereferenced; so are settings the encoder refuses
    assert lib.ire_encode_jpeg_base64_fit_ex(None, None, 1, 5, 7, None, 4096, None, 60, 2) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_jpeg_base64_fit_device_ex(None, None, 1, 5, 7, 21, 105, None, 4096, None, 60, 2, None) == _lib.IRE_ERR_INVALID_INPUT
