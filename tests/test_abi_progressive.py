"""The progressive decoder's part of the C ABI, on the CPU: IRE_FLAG_DECODE_PROGRESSIVE is a known bit of ire_config.flags and no
result format, ire_decode_jpeg_plan_ex is exported, declared for node and pure host code.

The flag is bit 32, not 16: tests/test_jpeg_model.py::test_abi_symbols_and_flag holds ire_init to refusing 16 and 24 as unknown bits,
and existing tests stay as they are; so 16 stays unknown (asserted below) and the cases here are written with the flag's name."""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_prog_writer as writer      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _init(flags):
    """ire_init with these flags -> (status, message): without a GPU a VALID configuration fails later, with another message"""
    lib = _lib.load()
    cfg = _lib.IreConfig()
    cfg.struct_size = ctypes.sizeof(_lib.IreConfig)
    cfg.device_index = 0
    cfg.max_batch = 1
    cfg.flags = flags
    out = ctypes.c_void_p()
    rc = lib.ire_init(ctypes.byref(cfg), ctypes.byref(out))
    msg = (lib.ire_last_error() or b"").decode()
    if rc == 0:
        lib.ire_shutdown(out)
    return rc, msg


def test_the_flag_is_known_and_no_result_format():
    P = _lib.IRE_FLAG_DECODE_PROGRESSIVE
    assert P == 32
    for flags in (P, P | 1, P | 4, P | 8):
        rc, msg = _init(flags)
        assert "ire_config.flags" not in msg, (flags, msg)
    rc, msg = _init(1 | 4)
    assert rc == _lib.IRE_ERR_INVALID_INPUT and "two result formats" in msg
    rc, msg = _init(P | 1 | 4)
    assert rc == _lib.IRE_ERR_INVALID_INPUT and "two result formats" in msg
    rc, msg = _init(2)
    assert rc == _lib.IRE_ERR_INVALID_INPUT and "unknown bits" in msg
    for unknown in (16, 24, 64, P | 16):
        rc, msg = _init(unknown)
        assert rc == _lib.IRE_ERR_INVALID_INPUT and "unknown bits" in msg, unknown
    assert _lib.load().ire_abi_version() == 3


def test_the_plan_entry_is_exported_declared_and_needs_no_engine():
    lib = _lib.load()
    assert hasattr(lib, "ire_decode_jpeg_plan_ex")
    header = open(os.path.join(ROOT, "include", "ire.h")).read()
    assert re.search(r"#define IRE_FLAG_DECODE_PROGRESSIVE 32u", header) and re.search(r"#define IRE_DECODE_ACCEPT_PROGRESSIVE 1u", header)
    assert "int ire_decode_jpeg_plan_ex(const uint8_t* file, size_t bytes, uint32_t accept, int* out_h, int* out_w, int* out_sampling, int* out_nscans);" in header
    assert int(re.search(r"#define IRE_DECODE_MAX_SCANS (\d+)", header).group(1)) == _lib.IRE_DECODE_MAX_SCANS
    ffi = open(os.path.join(ROOT, "image_restoration_platform_amd", "node", "ire_ffi.mjs")).read()
    assert "ire_decode_jpeg_plan_ex: ['int', [P, 'size_t', 'int', P, P, P, P]]" in ffi
    data = writer.pillow_progressive(cases.noise(13, 17, 5), 85, 2)
    h, w, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ire_decode_jpeg_plan_ex(data, len(data), 1, ctypes.byref(h), ctypes.byref(w), ctypes.byref(s), ctypes.byref(k)) == 0
    assert (h.value, w.value, s.value, k.value) == (13, 17, 2, 10)
    assert lib.ire_decode_jpeg_plan_ex(data, len(data), 0, None, None, None, None) == _lib.IRE_ERR_INVALID_INPUT
    assert "progressive JPEG (SOF2): not decoded on the device" in lib.ire_last_error().decode()
    assert lib.ire_decode_jpeg_plan(data, len(data), None, None, None) == _lib.IRE_ERR_INVALID_INPUT
