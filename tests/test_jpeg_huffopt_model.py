"""JPEG results with optimised Huffman tables, without a GPU: the model (tests/jpeg_huffopt_model.py) against libjpeg-turbo's own file
(Pillow, optimize=True) byte for byte; csrc/jpeg_huff_core.hpp -- the table builder the kernel runs, its lanes as a loop -- and the
any-table bounds and heads of csrc/jpeg_tables.hpp against the model, as a stand-alone program under the address and
undefined-behaviour sanitizers; and the C ABI: the new symbols, the flag, the bound."""
import ctypes
import functools
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_huffopt_cases as cases      # noqa: E402
import jpeg_huffopt_model as model      # noqa: E402
import jpeg_opt_model as opt            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from image_restoration_platform_amd import _lib      # noqa: E402


def pillow_file(px, quality, sampling):
    from PIL import Image, ImageFile
    bio = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 22      # (with optimize=True Pillow's encoder needs the whole file in one buffer; its own guess is too small for noise at quality 100)
    try:
        Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=quality, subsampling=sampling, optimize=True, restart_marker_blocks=opt.R_OF[sampling])
    finally:
        ImageFile.MAXBLOCK = keep
    return bio.getvalue()


@functools.lru_cache(maxsize=None)
def model_file(name, q, s):
    return model.jpeg_file(cases.image(name), q, s)


@pytest.mark.parametrize("name", cases.SMALL + cases.LARGE)
def test_model_equals_libjpeg_turbo(name):
    """Byte equality with Pillow's file for quality=q, subsampling=s, optimize=True, restart_marker_blocks=R."""
    px = cases.image(name)
    for n, q, s in cases.CASES:
        if n != name:
            continue
        f = model_file(name, q, s)
        assert f == pillow_file(px, q, s), (name, q, s)
        assert len(f) <= model.file_bound(px.shape[0], px.shape[1], q, s)
        assert len(model.header(px.shape[0], px.shape[1], q, s, model.tables_of(model.image_histograms(px, q, s)))) <= opt.HEADER_BYTES


def test_the_cases_reach_what_they_are_for():
    # the flat image: both AC tables hold EOB alone, a 1-bit code
    for s in cases.SAMPLINGS:
        tabs = model.tables_of(model.image_histograms(cases.image("flat"), 85, s))
        assert tabs[1] == ([1] + [0] * 15, [0]) and tabs[3] == ([1] + [0] * 15, [0])
        assert 290 <= len(model_file("flat", 85, s)) <= 296
    # ramp: RSTm wraps at 4:4:4
    assert -(-len(opt.mcus(cases.image("ramp"), 85, 0)) // 16) == 32
    # deep: the unlimited code lengths pass 16, so the limiting loop runs
    name, q, s = cases.DEEP
    longest = [model.gen_optimal_table(h)[2] for h in model.image_histograms(cases.image(name), q, s)]
    assert max(longest) > 16, longest
    assert model.gen_optimal_table(cases.synthetic_histograms()["fib30"])[2] >= 28      # (31 entries with the pseudo-symbol: a chain nearly as deep as it is long)
    # the tie rule: of two equal counts the LARGER index is taken first, to join the pseudo-symbol two levels down; the smaller symbol gets 1 bit
    assert model.gen_optimal_table(cases.synthetic_histograms()["tie2"])[:2] == ([1, 1] + [0] * 14, [0x03, 0x21])


def test_bounds():
    assert model.block_bits_any(0, 100) == 1665 and model.RAW_ANY == 9990
    for s in cases.SAMPLINGS:
        bits = [model.mcu_bits_any(q, s) for q in range(1, 101)]
        assert bits == sorted(bits)
        assert (opt.R_OF[s] * bits[-1] + 7) // 8 <= model.RAW_ANY
        for q in (1, 50, 85, 100):
            assert model.mcu_bits_any(q, s) >= opt.mcu_bits_max(q, s)      # the fixed tables are tables
    # under ANY table: every symbol at 16 bits still fits
    name, q, s = cases.DEEP
    ms = opt.mcus(cases.image(name), q, s)
    worst = max(sum(16 + nv for *_, nv in model.interval_symbols(iv, s)) for iv in model.intervals_of(ms, s))
    assert (worst + 7) // 8 <= model.RAW_ANY


@functools.lru_cache(maxsize=None)
def _exe(tmp):
    exe = os.path.join(tmp, "jpeg_huffopt_dump")
    src = os.path.join(ROOT, "tests", "native", "jpeg_huffopt_dump.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    return dict(line.split(": ", 1) for line in r.stdout.splitlines())


def _t_line(name, h):
    return "T %s %s\n" % (name, " ".join(str(int(c)) for c in h))


def _check_table(got, name, h):
    longest, n, bits, vals = re.fullmatch(r"(\d+) (\d+) \|((?: \d+)*) \|((?: \d+)*)", got["T " + name]).groups()
    mb, mv, ml = model.gen_optimal_table(h)
    assert (int(longest), int(n), [int(v) for v in bits.split()], [int(v) for v in vals.split()]) == (ml, len(mv), mb, mv), name


def test_native_against_the_model(tmp_path):
    """The shared table builder (the kernel's lane algorithm, lanes as a loop), the any-table bounds and class rule for all 200
    settings, and the heads, compiled alone with -fsanitize=address,undefined."""
    exe = _exe(str(tmp_path))
    hws = [(1, 1), (5, 7), (45, 37), (1024, 1024), (8192, 8192), (8192, 1), (1, 8192)]
    text = "B\n" + "".join("F %d %d %d %d\n" % (h, w, q, s) for h, w in hws for q in cases.QUALITIES for s in cases.SAMPLINGS)
    synth = cases.synthetic_histograms()
    text += "".join(_t_line(k, h) for k, h in synth.items())
    real = [(n, q, s) for n, q, s in cases.CASES if (q, s) in ((85, 0), (100, 0), (85, 2), (1, 2))]
    for n, q, s in real:
        px = cases.image(n)
        for t, h in enumerate(model.image_histograms(px, q, s)):
            text += _t_line("%s_%d_%d_%d" % (n, q, s, t), h)
        text += "H %d %d %d %d\n" % (px.shape[0], px.shape[1], q, s)
    got = _run(exe, text)
    for q in range(1, 101):
        for s in cases.SAMPLINGS:
            mb = model.mcu_bits_any(q, s)
            assert got["B %d %d" % (q, s)] == "%d %d 1" % (mb, (opt.R_OF[s] * mb + 7) // 8), (q, s)
    for h, w in hws:
        for q in cases.QUALITIES:
            for s in cases.SAMPLINGS:
                assert got["F %d %d %d %d" % (h, w, q, s)] == "%d %d" % (model.file_bound(h, w, q, s), model.base64_bound(h, w, q, s))
    for k, h in synth.items():
        _check_table(got, k, h)
    for n, q, s in real:
        px = cases.image(n)
        hist = model.image_histograms(px, q, s)
        for t, h in enumerate(hist):
            _check_table(got, "%s_%d_%d_%d" % (n, q, s, t), h)
        head = model.header(px.shape[0], px.shape[1], q, s, model.tables_of(hist))
        assert got["H %d %d %d %d" % (px.shape[0], px.shape[1], q, s)] == "%d %s" % (len(head), head.hex()), (n, q, s)
        # the bound is never below the model's actual file
        assert model.file_bound(px.shape[0], px.shape[1], q, s) >= len(model_file(n, q, s))


def test_abi():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ("ire_jpeg_optimized_base64_bound", "ire_encode_jpeg_optimized_base64_fit_device", "ire_encode_jpeg_optimized_base64_fit", "ire_debug_jpeg_huffman")
    ffi = open(os.path.join(ROOT, "image_restoration_platform_amd", "node", "ire_ffi.mjs")).read()
    for name in names:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in ffi, name
    assert _lib.IRE_FLAG_JPEG_OPTIMIZE == 128
    lib = _lib.load()
    assert ctypes.sizeof(_lib.IreConfig) == 48 and lib.ire_abi_version() == 3
    import torch
    accepted = _lib.IRE_OK if torch.cuda.is_available() else _lib.IRE_ERR_UNAVAILABLE      # as far as the device check

    def init(flags, quality=0, sampling=0):
        h = ctypes.c_void_p()
        cfg = _lib.IreConfig()
        cfg.struct_size, cfg.max_batch, cfg.flags, cfg.jpeg_quality, cfg.jpeg_sampling = ctypes.sizeof(_lib.IreConfig), 2, flags, quality, sampling
        st = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
        err = lib.ire_last_error()
        if st == _lib.IRE_OK:
            lib.ire_shutdown(h)
        return st, err

    assert init(_lib.IRE_FLAG_RESULT_JPEG | _lib.IRE_FLAG_JPEG_OPTIMIZE)[0] == accepted
    assert init(_lib.IRE_FLAG_RESULT_JPEG | _lib.IRE_FLAG_JPEG_OPTIMIZE | _lib.IRE_FLAG_DECODE_PROGRESSIVE, 60, 2)[0] == accepted
    for flags in (128, 128 | _lib.IRE_FLAG_RESULT_PNG_BASE64, 128 | _lib.IRE_FLAG_RESULT_PNG_DEFLATE, 128 | _lib.IRE_FLAG_DECODE_PROGRESSIVE):
        st, err = init(flags)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"invalid" in err and b"IRE_FLAG_RESULT_JPEG" in err, (flags, err)
    for bits in (16, 24, 64, 2, 8 | 16, 8 | 128 | 64):
        st, err = init(bits)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"unknown bits" in err, (bits, err)
    # the bound: the model's; 0 for what is refused
    for h, w in ((1, 1), (5, 7), (45, 37), (1024, 1024), (8192, 8192)):
        for q, s in ((1, 0), (60, 2), (85, 0), (100, 2), (100, 0)):
            assert lib.ire_jpeg_optimized_base64_bound(h, w, q, s) == model.base64_bound(h, w, q, s) >= lib.ire_jpeg_base64_bound_ex(h, w, q, s) > 0
        assert lib.ire_jpeg_optimized_base64_bound(h, w, 0, 0) == model.base64_bound(h, w, 85, 0)
    for h, w, q, s in ((0, 8, 85, 0), (8, 8193, 85, 2), (8, 8, 101, 0), (8, 8, -1, 0), (8, 8, 85, 1), (8, 8, 85, 3), (8, 8, 85, -2)):
        assert lib.ire_jpeg_optimized_base64_bound(h, w, q, s) == 0, (h, w, q, s)
    # null handles are refused, not dereferenced
    assert lib.ire_encode_jpeg_optimized_base64_fit(None, None, 1, 5, 7, None, 4096, None, 60, 2) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_jpeg_optimized_base64_fit_device(None, None, 1, 5, 7, 21, 105, None, 4096, None, 60, 2, None) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_debug_jpeg_huffman(None, None, 1, None, None) == _lib.IRE_ERR_INVALID_INPUT
