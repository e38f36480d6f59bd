"""The compressing PNG encoder without a GPU: the Python model of the format (tests/png_deflate_model.py) held to the published
formats by independent decoders (zlib's inflater, PIL's PNG reader, the chunk CRCs), the 15-bit limit, the worst-case bound, the
size condition against zlib's own Huffman-only stream, and the C ABI's new symbols and flag."""
import ctypes
import heapq
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_deflate_cases as cases      # noqa: E402
import png_deflate_model as model      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402


def chunks(f):
    """[(type, payload)] of a PNG file; every chunk's CRC is verified."""
    assert f[:8] == b"\x89PNG\r\n\x1a\n"
    out, o = [], 8
    while o < len(f):
        n, = struct.unpack(">I", f[o:o + 4])
        kind, payload = f[o + 4:o + 8], f[o + 8:o + 8 + n]
        crc, = struct.unpack(">I", f[o + 8 + n:o + 12 + n])
        assert zlib.crc32(kind + payload) & 0xFFFFFFFF == crc, kind
        out.append((kind, payload))
        o += 12 + n
    assert o == len(f)
    return out


def check_file(f, px):
    """the file against independent decoders; returns the IDAT payload"""
    from PIL import Image
    ch = chunks(f)
    assert [k for k, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert zlib.decompress(ch[1][1]) == model.paeth_filter(px)
    got = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
    assert got.shape == px.shape and (got == px).all()
    return ch[1][1]


@pytest.fixture(scope="module")
def all_cases():
    d = dict(cases.shape_cases())
    d["fibonacci"] = cases.fibonacci_image()
    d["skewed"] = cases.skewed_image()
    for r, seed in cases.MOD3_SEEDS.items():
        d["mod3_%d" % r] = cases.noise(6, 5, seed)
    return {k: (px, model.png_file(px)) for k, px in d.items()}


def huffman_cost(counts):
    h = [c for c in counts if c > 0]
    heapq.heapify(h)
    total = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        total += a + b
        heapq.heappush(h, a + b)
    return total


def test_model_files_decode_with_independent_decoders(all_cases):
    for name, (px, f) in all_cases.items():
        check_file(f, px)
    # the block structure the shapes were chosen for
    n = {k: len(model.blocks_of(model.paeth_filter(px))) for k, (px, _) in all_cases.items()}
    assert n["120x100"] == 2 and 32768 % (1 + 3 * 100) != 0          # a scanline straddles the boundary
    assert n["8192x1"] == 1 and 8192 * 4 == model.BLOCK and n["4096x5"] == 2 and 4096 * 16 == 2 * model.BLOCK
    assert n["random264x200"] == 5 and n["1x1"] == 1


def test_fifteen_bit_limit(all_cases):
    for name, counts, values in (("fibonacci", cases.FIB, cases.FIB_VALUES), ("skewed", cases.SKEW, cases.SKEW_VALUES)):
        px, f = all_cases[name]
        stream = model.paeth_filter(px)
        hist = np.bincount(np.frombuffer(stream, np.uint8), minlength=256)
        assert {v: int(hist[v]) for v in values} == dict(zip(values, counts)) and hist.sum() == sum(counts) < model.BLOCK
        lit, cl = model.block_lengths(stream)
        for lens, limit in ((lit, 15), (cl, 7)):
            assert max(lens) <= limit
            assert sum(2 ** (limit - l) for l in lens if l) == 2 ** limit            # Kraft with equality
        check_file(f, px)
    # on the skewed histogram the limit binds: the unlimited tree is deeper, so the limited code must cost more, and it uses 15 bits
    full = cases.SKEW + [1]
    lens = model.limited_lengths(full, 15)
    assert max(lens) == 15 and sum(c * l for c, l in zip(full, lens)) > huffman_cost(full)
    assert max(model.limited_lengths(full, 32)) == 18


def test_code_builder_is_optimal_where_that_can_be_checked():
    rng = np.random.default_rng(3)
    for _ in range(300):                    # no limit in the way: the cost is Huffman's
        n = int(rng.integers(2, 60))
        c = rng.integers(0, 40, n).tolist()
        if sum(1 for x in c if x) < 2:
            continue
        lens = model.limited_lengths(c, 30)
        assert sum(a * b for a, b in zip(c, lens)) == huffman_cost(c)
        assert all((l > 0) == (x > 0) for l, x in zip(lens, c))
    for _ in range(200):                    # a tight limit, few symbols: against every complete assignment (brute force)
        n = int(rng.integers(2, 7))
        c = sorted(rng.integers(1, 50, n).tolist(), reverse=True)
        limit = int(rng.integers(max(1, (n - 1).bit_length()), 4))

        def best(k, budget, prev):         # ascending lengths for descending counts, Kraft budget in units of 2^-limit
            if k == n:
                return 0 if budget >= 0 else None
            b = None
            for l in range(prev, limit + 1):
                rest = best(k + 1, budget - 2 ** (limit - l), l) if budget - 2 ** (limit - l) >= 0 else None
                if rest is not None and (b is None or c[k] * l + rest < b):
                    b = c[k] * l + rest
            return b
        lens = model.limited_lengths(c, limit)
        assert max(lens) <= limit and sum(a * b for a, b in zip(c, lens)) == best(0, 2 ** limit, 1), (c, limit, lens)


def adversarial_histograms():
    yield "all equal", [128] * 256 + [1]
    yield "two symbols", [0] * 255 + [32768, 1]
    yield "geometric", [max(1, 32768 >> (k // 2)) if k < 40 else 0 for k in range(256)] + [1]
    yield "one heavy, the rest once", [32768 - 255] + [1] * 255 + [1]
    yield "skewed", cases.SKEW + [0] * (256 - len(cases.SKEW)) + [1]
    yield "fibonacci", cases.FIB + [0] * (256 - len(cases.FIB)) + [1]
    rng = np.random.default_rng(9)
    for k in range(20):
        c = np.zeros(257, np.int64)
        used = rng.choice(256, int(rng.integers(1, 257)), replace=False)
        c[used] = rng.integers(1, 1 + 2 ** int(rng.integers(1, 12)), len(used))
        c[256] = 1
        yield "random %d" % k, c.tolist()


def test_bound(all_cases):
    lib = _lib.load()
    for name, (px, f) in all_cases.items():
        h, w, _ = px.shape
        assert len(f) <= model.file_bound(h, w), name
        assert lib.ire_png_deflate_base64_bound(h, w) == model.base64_bound(h, w) >= (len(f) + 2) // 3 * 4
    for name, hist in adversarial_histograms():
        n = sum(hist) - 1
        if n > model.BLOCK:
            hist = [c * model.BLOCK // (n + 300) if c > 1 else c for c in hist]
            n = sum(hist) - 1
        lit = model.limited_lengths(hist, 15)
        assert max(lit) <= 15 and sum(2 ** (15 - l) for l in lit if l) == 2 ** 15, name
        data = sum(c * l for c, l in zip(hist, lit))
        assert data <= 9 * (n + 1), name                                     # no worse than the flat code
        clh = [0] * 19
        for l in lit + [1, 1]:
            clh[l] += 1
        cl = model.limited_lengths(clh, 7)
        header = 17 + 3 * 19 + sum(clh[s] * cl[s] for s in range(19))
        assert header <= model.HEADER_BITS_MAX
        assert (header + data + 3 + 7) // 8 + 4 <= model.block_bound(n), name
    for h, w in [(1, 1), (5, 7), (64, 64), (750, 1000), (1024, 1024), (1365, 2048), (8192, 8192)]:
        b = lib.ire_png_deflate_base64_bound(h, w)
        assert b == model.base64_bound(h, w)
        assert b >= lib.ire_png_base64_bytes_fit(h, w) > 0                   # a stored stream always fits what sizes the buffers
        assert b <= lib.ire_png_base64_bytes_fit(h, w) * 9 // 8 + 4 * 400 * ((h * (1 + 3 * w) + 32767) // 32768)
    for h, w in [(0, 8), (8, 0), (-1, 8), (8, -8), (8193, 8), (8, 8193), (0, 0)]:
        assert lib.ire_png_deflate_base64_bound(h, w) == 0, (h, w)


def test_size_condition_against_zlib_huffman_only(all_cases):
    """len(model IDAT) <= len(zlib Z_HUFFMAN_ONLY stream of the same filtered bytes) + 256 per block: per-block optimal codes cannot
    lose materially to zlib's blocks, and 256 B covers a dynamic block header."""
    checked = 0
    for name, (px, f) in all_cases.items():
        stream = model.paeth_filter(px)
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        ref = co.compress(stream) + co.flush()
        idat = chunks(f)[1][1]
        nblocks = (len(stream) + model.BLOCK - 1) // model.BLOCK
        print("%-14s model %7d  zlib huffman-only %7d  blocks %d" % (name, len(idat), len(ref), nblocks))
        assert len(idat) <= len(ref) + 256 * nblocks, name
        checked += 1
    assert checked == len(all_cases)


def test_file_length_mod_3_seeds(all_cases):
    import base64
    for r in (0, 1, 2):
        px, f = all_cases["mod3_%d" % r]
        assert len(f) % 3 == r
        assert model.png_base64(px) == base64.b64encode(f) and model.png_base64(px).count(b"=") == (3 - r) % 3


def test_abi_symbols_and_flag():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ire_png_deflate_base64_bound", "ire_encode_png_deflate_base64_fit_device", "ire_encode_png_deflate_base64_fit", "ire_poll_text"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert _lib.IRE_FLAG_RESULT_PNG_DEFLATE == 4
    import torch
    h = ctypes.c_void_p()
    cfg = _lib.IreConfig()
    cfg.struct_size = ctypes.sizeof(_lib.IreConfig)
    cfg.max_batch = 2
    for bad in (6, 5):                       # 2 is no flag; the two result formats exclude each other
        cfg.flags = bad
        assert lib.ire_init(ctypes.byref(cfg), ctypes.byref(h)) == _lib.IRE_ERR_INVALID_INPUT
        assert b"flags" in lib.ire_last_error()
    cfg.flags = 4                            # accepted as far as the device check
    st = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
    if torch.cuda.is_available():
        assert st == _lib.IRE_OK, lib.ire_last_error()
        lib.ire_shutdown(h)
    else:
        assert st == _lib.IRE_ERR_UNAVAILABLE and b"flags" not in lib.ire_last_error()
    # null handles are rejected, not dereferenced
    n = ctypes.c_size_t(0)
    assert lib.ire_poll_text(None, None, 0, None, 0, ctypes.byref(n), None, None) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_png_deflate_base64_fit(None, None, 1, 5, 7, None, 1024, None) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_png_deflate_base64_fit_device(None, None, 1, 5, 7, 21, 105, None, 1024, None, None) == _lib.IRE_ERR_INVALID_INPUT
