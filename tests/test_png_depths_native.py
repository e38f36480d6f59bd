"""The PNG forms of IRE_FLAG_DECODE_PNG_ALL on the CPU, before any of them reaches a GPU: 1, 2, 4 and 16 bits per sample and Adam7.
The plan through the C ABI (every accepted form with its depth and interlace, every new refusal with a word of its reason, the SAME
files refused with the old reasons without the accept bit, the flag rules); tests/native/png_any_sim.cpp -- csrc/png_adam7_core.hpp
with the lanes of csrc/png_dec.hip's png_unfilter_any_kernel as a loop -- built plain and under ASan + UBSan and run directly: its
RGB equals Pillow's and its scanlines equal zlib.decompress on every case of tests/png_depth_cases.py; truncations and mutations end
in a refusal or a status, status 0 exactly where zlib yields the passes' scanlines with filter bytes 0..4.  With "--poison BYTE"
(tests/native/png_sim.hpp: dirty LDS and scratch) every line, and the pixels and scanlines of every file with status 0, stay the same."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as old_cases      # noqa: E402
import png_depth_cases as cases    # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import decode_png_plan_ex_reason, decode_png_plan_reason, upload_plan_reason      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
ALL = cases.ACCEPT_ALL


# ---- the plan and the flags, through the ABI ------------------------------------------------------------------------------------------
def test_constants():
    assert _lib.IRE_FLAG_DECODE_PNG_ALL == cases.FLAG_PNG_ALL == 8192 and _lib.IRE_DECODE_ACCEPT_PNG_ALL == ALL == 32
    hdr = open(os.path.join(ROOT, "include", "ire.h")).read()
    assert "#define IRE_FLAG_DECODE_PNG_ALL 8192u" in hdr and "#define IRE_DECODE_ACCEPT_PNG_ALL 32u" in hdr


def test_every_accepted_form_is_planned_with_its_depth_and_interlace():
    files = cases.accept_cases()
    assert len(files) >= 180
    seen = set()
    for name, data in files.items():
        h, w, ct, d, lace = cases.head_of(data)
        plan, why = decode_png_plan_ex_reason(data, ALL)
        assert plan == (h, w, ct, d, lace), (name, plan, why)
        seen.add((ct, d, lace))
        # without the bit: the reason the file always got, from both plan entries
        for got in (decode_png_plan_ex_reason(data, 0), decode_png_plan_reason(data)):
            assert got[0] is None and got[1].startswith("invalid: PNG ") and cases.old_reason_word(ct, d, lace) in got[1], (name, got)
    assert seen >= {(ct, d, lace) for ct, d in cases.FORMS for lace in (0, 1) if (d, lace) != (8, 0)}


def test_the_old_form_plans_the_same_with_and_without_the_bit():
    for name, data in list(old_cases.shape_cases().items())[:12]:
        a, b = decode_png_plan_ex_reason(data, 0), decode_png_plan_ex_reason(data, ALL)
        assert a == b and a[0][3:] == (8, 0) and a[0][:3] == decode_png_plan_reason(data)[0], name
    for name, (data, word) in old_cases.refused_cases().items():
        if name in ("depth16", "depth4", "adam7"):          # (forms the bit admits; their stream is that of another form)
            continue
        for accept in (0, ALL):
            plan, why = decode_png_plan_ex_reason(data, accept)
            assert plan is None and word in why, (name, accept, why)


def test_new_refusals_and_their_old_reasons():
    for name, (data, word, old_word) in cases.refused_cases().items():
        plan, why = decode_png_plan_ex_reason(data, ALL)
        assert plan is None and why.startswith("invalid: PNG ") and word in why, (name, why)
        plan, why = decode_png_plan_ex_reason(data, 0)
        assert plan is None and old_word in why, (name, why)
        assert decode_png_plan_reason(data)[1] == why
    assert "host codecs disagree" in decode_png_plan_ex_reason(cases.refused_cases()["grey16"][0], ALL)[1]


def test_pillow_clips_16_bit_grey_which_is_why_it_stays_refused():
    s = np.array([[[0x0100], [0x0012], [0x00FF], [0xFFFF]]], np.uint32)
    data = cases.png_any(s, 0, 16)
    assert decode_png_plan_ex_reason(data, ALL)[0] is None
    assert cases.pil_rgb(data)[0, :, 0].tolist() == [255, 18, 255, 255]          # not the high byte (1, 0, 0, 255)


def test_accept_bits_of_the_plans():
    lib = _lib.load()
    data = cases.make(5, 3, 0, 4, 1)
    for bad in (1, 2, 4, 8, 16, 64, 33):
        assert lib.ire_decode_png_plan_ex(data, len(data), bad, None, None, None, None, None) == _lib.IRE_ERR_INVALID_INPUT
        assert b"unknown accept bits" in lib.ire_last_error()
    assert lib.ire_decode_png_plan_ex(data, len(data), ALL, None, None, None, None, None) == 0          # every output pointer may be null
    assert lib.ire_decode_png_plan_ex(None, 0, ALL, None, None, None, None, None) == _lib.IRE_ERR_INVALID_INPUT
    # ire_upload_plan: 32 is known beside 16; 2 and 8 are still unknown
    png, png_all = _lib.IRE_DECODE_ACCEPT_PNG, _lib.IRE_DECODE_ACCEPT_PNG | ALL
    data = cases.make(24, 20, 0, 4, 1)
    plan, why = upload_plan_reason(data, 64, png_all)
    assert plan is not None and plan[:2] == (24, 20), why
    plan, why = upload_plan_reason(data, 64, png)
    assert plan is None and "bit depth other than 8" in why
    for bad in (2, 8, png_all | 2, png_all | 8):
        plan, why = upload_plan_reason(data, 64, bad)
        assert plan is None and "unknown accept bits" in why, (bad, why)
    plan, why = upload_plan_reason(data, 64, ALL)
    assert plan is None and "IRE_DECODE_ACCEPT_PNG" in why
    # the orientation of a new form's eXIf chunk reaches the upload plan
    import png_writer as pw
    turned = cases.make(24, 20, 2, 16, 1, smooth=True, before_idat=[pw.exif_chunk(6)])
    assert upload_plan_reason(turned, 64, png_all)[0][:3] == (24, 20, 6)
    # and the room rule holds for the new forms: 16-bit noise does not compress below its 8-bit pixels
    noise = cases.png_any(np.random.default_rng(3).integers(0, 65536, (24, 20, 3)).astype(np.uint32), 2, 16)
    plan, why = upload_plan_reason(noise, 64, png_all)
    assert plan is None and "may be larger than its fitted pixels" in why, why


def _init(flags):
    lib = _lib.load()
    h = ctypes.c_void_p()
    cfg = _lib.IreConfig()
    cfg.struct_size = ctypes.sizeof(_lib.IreConfig)
    cfg.max_batch = 8
    cfg.flags = flags
    rc = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
    why = (lib.ire_last_error() or b"").decode()
    if rc == 0:
        lib.ire_shutdown(h)
    return rc, why


def test_flag_rules():
    rc, why = _init(cases.FLAG_PNG_ALL)
    assert rc == _lib.IRE_ERR_INVALID_INPUT and "invalid" in why and "IRE_FLAG_DECODE_PNG" in why and "unknown bits" not in why
    rc, why = _init(cases.FLAG_PNG_ALL | cases.FLAG_PNG)          # accepted as far as the device check
    assert rc == 0 or (rc == _lib.IRE_ERR_UNAVAILABLE and "flags" not in why), (rc, why)
    for bit in (2, 16, 64, 512, 4096):
        rc, why = _init(bit | cases.FLAG_PNG | cases.FLAG_PNG_ALL)
        assert rc == _lib.IRE_ERR_INVALID_INPUT and "unknown bits" in why, (bit, why)


# ---- the decoder's CPU form ---------------------------------------------------------------------------------------------------------
def _build(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + [os.path.join(NATIVE, "png_any_sim.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("png_any_sim")
    return {"tmp": tmp, "sim": _build(tmp, "sim", ["-O2"]), "sim_san": _build(tmp, "sim_san", ["-O1", "-fsanitize=address,undefined"])}


def _dump(ex, exe, data, flags=ALL, poison=None):
    tmp = ex["tmp"]
    src, rgb, scan = str(tmp / "in.png"), str(tmp / "rgb.bin"), str(tmp / "scan.bin")
    with open(src, "wb") as f:
        f.write(data)
    lines = _run(ex[exe], *(() if poison is None else ("--poison", str(poison))), "dump", src, rgb, scan, str(flags))
    if lines[0].startswith("refused "):
        return lines[0][len("refused "):]
    return [int(v) for v in lines[0].split()[1:]], int(lines[1].split()[1]), np.fromfile(rgb, np.uint8), np.fromfile(scan, np.uint8)


@pytest.fixture(scope="module")
def accept():
    return {name: (data, cases.pil_rgb(data)) for name, data in cases.accept_cases().items()}      # Pillow's pixels, computed once


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
@pytest.mark.parametrize("exe", ["sim", "sim_san"])
def test_pixels_equal_pillow_and_scanlines_equal_zlib(exes, accept, exe):
    for name, (data, want) in accept.items():
        got = _dump(exes, exe, data)
        assert not isinstance(got, str), (name, got)
        head, status, rgb, scan = got
        h, w, ct, d, lace = cases.head_of(data)
        assert (head[0], head[1], head[2], head[7], head[8]) == (h, w, ct, d, lace) and head[3] == max(1, cases.CHANNELS[ct] * d // 8) and status == 0, (name, head, status)
        assert scan.tobytes() == zlib.decompress(cases.idat_stream(data)) and len(scan) == cases.scan_bytes(h, w, ct, d, lace), name
        assert np.array_equal(rgb.reshape(want.shape), want), name
    # without the bit the same program refuses a file with the old reason
    name, (data, _) = next(iter(accept.items()))
    why = _dump(exes, exe, data, flags=0)
    assert isinstance(why, str) and cases.old_reason_word(*cases.head_of(data)[2:]) in why, why


def test_the_old_form_gives_the_same_bytes_through_the_new_program(exes):
    for name, data in list(old_cases.shape_cases().items()):
        head, status, rgb, _ = _dump(exes, "sim_san", data)
        want = old_cases.pil_rgb(data)
        assert status == 0 and head[7:] == [8, 0] and np.array_equal(rgb.reshape(want.shape), want), name


def test_a_filter_byte_of_5_on_a_pass_first_row_is_status_16(exes):
    bad, good = cases.bad_filter_adam7()
    assert _dump(exes, "sim_san", bad)[1] == 16 and _dump(exes, "sim_san", good)[1] == 0
    assert not cases.zlib_says_ok(cases.idat_stream(bad), cases.head_of(bad))[0]


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_what_lds_and_scratch_held(exes, byte):
    """every accepted case, the old form, the filter-byte-5 file, the refused files and both fuzz files' cuts and mutations, under the
    sanitizers with dirty LDS and scratch, against the plain program's unpoisoned run"""
    files = dict(cases.accept_cases())
    files.update({"old_" + k: v for k, v in old_cases.shape_cases().items()})
    files.update({"refused_" + k: v[0] for k, v in cases.refused_cases().items()})
    files["bad_filter"], files["good_filter"] = cases.bad_filter_adam7()
    for name, data in files.items():
        a, b = _dump(exes, "sim_san", data, poison=byte), _dump(exes, "sim", data)
        if isinstance(a, str) or isinstance(b, str):
            assert a == b, name
            continue
        assert a[0] == b[0] and a[1] == b[1], (name, a[:2], b[:2])
        if a[1] == 0:              # (what a flagged file leaves in its pixels is nobody's result)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name
    for which, good in cases.fuzz_files().items():
        src = str(exes["tmp"] / ("fuzz_poison_%s.png" % which))
        with open(src, "wb") as f:
            f.write(good)
        lines = _run(exes["sim_san"], "--poison", str(byte), "fuzz", src, str(cases.FUZZ_SEED), "200", str(ALL))
        assert len(lines) > 200 and lines == _run(exes["sim"], "fuzz", src, str(cases.FUZZ_SEED), "200", str(ALL)), which


@pytest.mark.parametrize("which", ["adam7_plte4", "rgb16"])
def test_truncations_and_mutations_under_the_sanitizers(exes, which):
    tmp = exes["tmp"]
    good = cases.fuzz_files()[which]
    src = str(tmp / ("fuzz_%s.png" % which))
    with open(src, "wb") as f:
        f.write(good)
    z, head = cases.idat_stream(good), cases.head_of(good)
    assert cases.zlib_says_ok(z, head) == (True, False)
    idat_end = good.index(b"IDAT") + 4 + len(z) + 4
    lines = _run(exes["sim_san"], "fuzz", src, str(cases.FUZZ_SEED), "200", str(ALL))
    assert lines == _run(exes["sim"], "fuzz", src, str(cases.FUZZ_SEED), "200", str(ALL))
    cuts = [l.split() for l in lines if l.startswith("cut ")]
    muts = [l.split() for l in lines if l.startswith("mut ")]
    assert len(cuts) == (len(good) + 9) // 10 and len(muts) == 200
    want = cases.pil_rgb(good)
    for f in cuts:
        assert f[2] == "refused" or (f[2:] == ["status", "0"] and int(f[1]) >= idat_end), f
        if f[2] != "refused":
            assert np.array_equal(cases.pil_rgb(good[:int(f[1])]), want), f
    rejected, statuses = 0, set()
    for f in muts:
        off, val = int(f[1]), int(f[2])
        bad = bytearray(z)
        assert bad[off] != val
        bad[off] = val
        ok, zlib_rejects = cases.zlib_says_ok(bytes(bad), head)
        rejected += zlib_rejects
        if f[3] == "refused":           # the zlib header's two bytes
            assert off < 2, f
            continue
        assert (int(f[4]) == 0) == ok, (f, ok)
        statuses.add(int(f[4]))
    print(which, "statuses", sorted(statuses), "zlib rejects", rejected)
    assert rejected >= 50
