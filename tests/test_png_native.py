"""csrc/png_parse.hpp and csrc/png_inflate_core.hpp on the CPU (tests/native/png_dec_sim.cpp and png_fuzz.cpp: the lane algorithm of
csrc/png_dec.hip with lanes as a loop), stand-alone programs built plain and under ASan + UBSan and run directly: the RGB equals
Pillow's and the filtered scanlines equal zlib.decompress on every case; truncations and mutations end in a refusal or a status with
no sanitizer report, and the status is 0 exactly where zlib decompresses the stream to exactly h * (1 + w * bpp) bytes whose filter
bytes are 0..4 -- before any PNG reaches a GPU.

With "--poison BYTE" the simulator's stand-ins for LDS and for device scratch that no launch clears (the inflate state, the scanlines,
the hand-off row, the pixels) start as that byte: every line printed, and the pixels and scanlines of every file with status 0, must
equal the unpoisoned run's, under the sanitizers."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as cases      # noqa: E402
import png_writer as pw        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _build(tmp, src, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + [os.path.join(NATIVE, src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("png_dec_sim")
    san = ["-O1", "-fsanitize=address,undefined"]
    return {"tmp": tmp, "sim": _build(tmp, "png_dec_sim.cpp", "sim", ["-O2"]), "sim_san": _build(tmp, "png_dec_sim.cpp", "sim_san", san),
            "fuzz": _build(tmp, "png_fuzz.cpp", "fuzz", ["-O2"]), "fuzz_san": _build(tmp, "png_fuzz.cpp", "fuzz_san", san)}


idat_stream = cases.idat_stream


def zlib_says_ok(z, head):
    """the three-part rule of status 0, with stdlib zlib"""
    h, w, bpp = head
    try:
        d = zlib.decompress(z)
    except zlib.error:
        return False, True
    stride = 1 + w * bpp
    return len(d) == h * stride and all(d[y * stride] <= 4 for y in range(h)), False


def _dump(ex, exe, data, flags=0, poison=None):
    tmp = ex["tmp"]
    src, rgb, scan = str(tmp / "in.png"), str(tmp / "rgb.bin"), str(tmp / "scan.bin")
    with open(src, "wb") as f:
        f.write(data)
    lines = _run(ex[exe], *(() if poison is None else ("--poison", str(poison))), "dump", src, rgb, scan, str(flags))
    if lines[0].startswith("refused "):
        return lines[0][len("refused "):]
    head = [int(v) for v in lines[0].split()[1:]]
    f = lines[1].split()
    return head, int(f[1]), int(f[3]), np.fromfile(rgb, np.uint8), np.fromfile(scan, np.uint8)


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
def test_pixels_equal_pillow_and_scanlines_equal_zlib(exes):
    acc = cases.accept_cases()
    rounds = {}
    for exe in ("sim", "sim_san"):
        for name, data in acc.items():
            got = _dump(exes, exe, data)
            assert not isinstance(got, str), (name, got)
            head, status, rounds[name], rgb, scan = got
            want = cases.pil_rgb(data)
            z, (h, w, bpp) = idat_stream(data)
            assert head[:2] == [h, w] and head[3] == bpp and status == 0, (name, head, status)
            assert np.array_equal(rgb.reshape(want.shape), want), name
            assert scan.tobytes() == zlib.decompress(z), name
    assert rounds["200x160_rgb"] > 3 and rounds["far258"] > 32768 // 256      # more than one round of the queue, a window of 32 KiB crossed


def test_refusals(exes):
    for name, (data, word) in cases.refused_cases().items():
        why = _dump(exes, "sim_san", data)
        assert isinstance(why, str) and why.startswith("invalid: PNG ") and word in why, (name, why)
    tagged = cases.make(6, 5, 2, before_idat=[pw.chunk(b"iCCP", b"x\x00\x00" + zlib.compress(b"profile"))])
    assert "iCCP" in _dump(exes, "sim_san", tagged, flags=4)
    assert not isinstance(_dump(exes, "sim_san", tagged), str)


def test_orientation_from_exif(exes):
    for o in range(1, 9):
        for be in (False, True):
            head = _dump(exes, "sim_san", cases.make(6, 5, 2, before_idat=[pw.exif_chunk(o, be)]))[0]
            assert head[4] == o
    for broken in (b"", b"II*\x00", b"XX*\x00\x08\x00\x00\x00", b"II*\x00\xff\xff\xff\x7f", b"MM\x00*\x00\x00\x00\x08\x00\x05"):
        head = _dump(exes, "sim_san", cases.make(6, 5, 2, before_idat=[pw.chunk(b"eXIf", broken)]))[0]
        assert head[4] == 1


def test_truncations_and_mutations_under_the_sanitizers(exes):
    tmp = exes["tmp"]
    good = cases.fuzz_file()
    src = str(tmp / "fuzz.png")
    with open(src, "wb") as f:
        f.write(good)
    z, head = idat_stream(good)
    idat_end = good.index(b"IDAT") + 4 + len(z) + 4
    lines = _run(exes["fuzz_san"], src, str(cases.FUZZ_SEED), "200")
    assert lines == _run(exes["fuzz"], src, str(cases.FUZZ_SEED), "200")
    cuts = [l.split() for l in lines if l.startswith("cut ")]
    muts = [l.split() for l in lines if l.startswith("mut ")]
    assert len(cuts) == (len(good) + 9) // 10 and len(muts) == 200
    for f in cuts:
        # a cut behind the last IDAT chunk may leave a whole image: accepted only where Pillow reads the same bytes to the same pixels
        assert f[2] == "refused" or (f[2:] == ["status", "0"] and int(f[1]) >= idat_end), f
        if f[2] != "refused":
            assert np.array_equal(cases.pil_rgb(good[:int(f[1])]), cases.pil_rgb(good)), f
    rejected, statuses = 0, {}
    for f in muts:
        off, val = int(f[1]), int(f[2])
        bad = bytearray(z)
        assert bad[off] != val
        bad[off] = val
        ok, zlib_rejects = zlib_says_ok(bytes(bad), head)
        rejected += zlib_rejects
        if f[3] == "refused":           # the zlib header's two bytes
            assert off < 2, f
            continue
        status = int(f[4])
        assert (status == 0) == ok, (f, ok)
        statuses.setdefault(status, (off, val))
    print("statuses", sorted(statuses), "zlib rejects", rejected)
    assert rejected >= 50



def test_corrupt_data_gets_ten_distinct_statuses(exes):
    """the files tests/test_png_decode_gpu.py sends to the device afterwards: each flagged here first, under the sanitizers"""
    statuses = {}
    for name, data in cases.corrupt_cases().items():
        got = _dump(exes, "sim_san", data)
        assert not isinstance(got, str), (name, got)
        z, head = idat_stream(data)
        assert got[1] != 0 and not zlib_says_ok(z, head)[0], (name, got[1])
        statuses[name] = got[1]
    print(statuses)
    assert len(set(statuses.values())) == 10


def _same(a, b, name):
    """two _dump results: the same refusal, or the same head and status and, at status 0, the same pixels and scanlines (what a flagged
    file leaves in its pixels is nobody's result: the caller is told to ignore them)"""
    if isinstance(a, str) or isinstance(b, str):
        assert a == b, name
        return
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], (name, a[:3], b[:3])
    if a[1] == 0:
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), name


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_what_lds_and_scratch_held(exes, byte):
    """this file's good cases, its refused and corrupt ones, and the cuts and mutations of the fuzz file, with dirty LDS and scratch"""
    files = dict(cases.accept_cases())
    files.update({"refused_" + k: v[0] for k, v in cases.refused_cases().items()})
    files.update({"corrupt_" + k: v for k, v in cases.corrupt_cases().items()})
    for name, data in files.items():
        _same(_dump(exes, "sim_san", data, poison=byte), _dump(exes, "sim", data), name)
    src = str(exes["tmp"] / "fuzz_poison.png")
    with open(src, "wb") as f:
        f.write(cases.fuzz_file())
    lines = _run(exes["fuzz_san"], "--poison", str(byte), src, str(cases.FUZZ_SEED), "200")
    assert len(lines) > 200 and lines == _run(exes["fuzz"], src, str(cases.FUZZ_SEED), "200")


def _pillow_reads(data, want):
    try:
        return np.array_equal(cases.pil_rgb(data), want)
    except Exception:      # noqa: BLE001 -- whatever Pillow raises, it did not decode the file
        return False


def test_no_cut_of_a_file_with_chunks_behind_idat_is_read_where_pillow_refuses(exes):
    """being stricter than Pillow is safe, being laxer is not: every file of behind_idat_cases cut at every byte from its IDAT on -- where
    the parser accepts and the decoder gives status 0, Pillow decodes the same bytes to the same pixels.  A cut inside the payload of a chunk
    behind IDAT, and a wrong CRC in front of IDAT, are refused; a clean end, a cut inside a chunk's header and a cut IEND are read."""
    tmp = exes["tmp"]
    want = cases.pixels(6, 5, 2)
    variants = []
    for name, data in cases.behind_idat_cases().items():
        for cut in range(data.index(b"IDAT"), len(data) + 1):
            variants.append((name, cut, data[:cut]))
    pack = str(tmp / "behind.bin")
    with open(pack, "wb") as f:
        for _, _, d in variants:
            f.write(struct.pack("<I", len(d)) + d)
    lines = _run(exes["sim_san"], "batch", pack)
    assert len(lines) == len(variants)
    read = {}
    for (name, cut, d), line in zip(variants, lines):
        if line == "status 0":
            read[(name, cut)] = True
            assert _pillow_reads(d, want), (name, cut, len(d))
    text = cases.behind_idat_cases()["text"]
    whole = len(text)
    assert len(read) >= 100
    assert ("text", whole) in read and ("text", whole - 2) in read              # whole; IEND without all of its CRC
    assert ("text", whole - 12 - 10) not in read and not _pillow_reads(text[:whole - 22], want)      # inside the tEXt payload
    assert ("text", whole - 12 - 35 + 5) in read                                # inside the tEXt chunk's eight header bytes
    assert not any(name == "crc_in_front" for name, _ in read)
