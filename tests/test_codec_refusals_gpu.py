"""What the text encoders' entries refuse, and with which words: every format (stored PNG, deflate PNG, JPEG), the host and the device
fit entry of each, through the raw C ABI (the Python wrappers check sizes before the library sees them).  The expected texts are
literals: one format's message must never borrow another's noun or bound.  After its refusals every entry still encodes, and its text
equals the Python model's (oracle/encode.py, tests/png_deflate_model.py, tests/jpeg_model.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_model      # noqa: E402
import png_deflate_model      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from oracle import encode as oenc      # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = {
    "png": dict(host="ire_encode_png_base64_fit", device="ire_encode_png_base64_fit_device", bound="ire_png_base64_bytes_fit", counted=False, model=oenc.png_base64,
                stride="invalid stride for the PNG encoder: smaller than ire_png_base64_bytes(h, w)",
                pitch="invalid pitch for the PNG encoder: rows or images overlap",
                device_args="invalid arguments to the PNG encoder (1..max_batch images)",
                device_size="invalid image size for the PNG encoder: height and width must be in 1..8192",
                host_null="invalid arguments to the PNG encoder: null buffer",
                host_args="invalid arguments to the PNG encoder (1..max_batch images, 1..8192 per side)"),
    "png_deflate": dict(host="ire_encode_png_deflate_base64_fit", device="ire_encode_png_deflate_base64_fit_device", bound="ire_png_deflate_base64_bound", counted=True,
                        model=png_deflate_model.png_base64,
                        stride="invalid stride for the PNG encoder: smaller than ire_png_deflate_base64_bound(h, w)",
                        pitch="invalid pitch for the PNG encoder: rows or images overlap",
                        device_args="invalid arguments to the PNG encoder (1..max_batch images)",
                        device_size="invalid image size for the PNG encoder: height and width must be in 1..8192",
                        host_null="invalid arguments to the PNG encoder: null buffer",
                        host_args="invalid arguments to the PNG encoder (1..max_batch images, 1..8192 per side)"),
    "jpeg": dict(host="ire_encode_jpeg_base64_fit", device="ire_encode_jpeg_base64_fit_device", bound="ire_jpeg_base64_bound", counted=True, model=jpeg_model.jpeg_base64,
                 stride="invalid stride for the JPEG encoder: smaller than ire_jpeg_base64_bound(h, w)",
                 pitch="invalid pitch for the JPEG encoder: rows or images overlap",
                 device_args="invalid arguments to the JPEG encoder (1..max_batch images)",
                 device_size="invalid image size for the JPEG encoder: height and width must be in 1..8192",
                 host_null="invalid arguments to the JPEG encoder: null buffer",
                 host_args="invalid arguments to the JPEG encoder (1..max_batch images, 1..8192 per side)"),
}


@pytest.fixture(scope="module")
def inputs():
    """(one 1 x 1 image, a batch of two 9 x 17 images)"""
    rng = np.random.default_rng(917)
    return rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (2, 9, 17, 3), dtype=np.uint8)


class _Entry:
    """One entry of one format on buffers that hold a whole batch of `px` at the format's bound: call() takes overrides of single arguments."""

    def __init__(self, engine, fmt, device, px):
        import torch
        self.eng, self.f, self.device, self.px = engine, FORMATS[fmt], device, px
        self.n, self.h, self.w = px.shape[:3]
        self.bound = int(getattr(engine._lib, self.f["bound"])(self.h, self.w))
        if device:
            self.rgb = torch.from_numpy(px).cuda()
            self.chars = torch.zeros((self.n, self.bound), dtype=torch.uint8, device="cuda")
            self.lens = torch.zeros(self.n, dtype=torch.int64, device="cuda")
            self.ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        else:
            self.rgb, self.chars, self.lens = px, np.zeros((self.n, self.bound), np.uint8), np.zeros(self.n, np.uint64)
            self.ptr = lambda a: ctypes.c_void_p(a.ctypes.data)

    def call(self, **over):
        import torch
        a = dict(rgb=self.ptr(self.rgb), n=self.n, h=self.h, w=self.w, row_pitch=3 * self.w, image_pitch=3 * self.w * self.h, chars=self.ptr(self.chars),
                 stride=self.bound, lens=self.ptr(self.lens))
        a.update(over)
        lens = [a["lens"]] if self.f["counted"] else []
        if self.device:
            st = getattr(self.eng._lib, self.f["device"])(self.eng._h, a["rgb"], a["n"], a["h"], a["w"], a["row_pitch"], a["image_pitch"], a["chars"], a["stride"], *lens,
                                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        else:
            st = getattr(self.eng._lib, self.f["host"])(self.eng._h, a["rgb"], a["n"], a["h"], a["w"], a["chars"], a["stride"], *lens)
        return st, (self.eng._lib.ire_last_error() or b"").decode()

    def texts(self):
        chars = self.chars.cpu().numpy() if self.device else self.chars
        lens = (self.lens.cpu().numpy() if self.device else self.lens) if self.f["counted"] else [self.bound] * self.n
        return [chars[i, :int(lens[i])].tobytes() for i in range(self.n)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_refusals_and_the_call_after_them(engine, inputs, fmt, device):
    f = FORMATS[fmt]
    refused = []

    def refuse(e, want, **over):
        st, msg = e.call(**over)
        print("%-11s %-6s %-28s -> %d %s" % (fmt, "device" if device else "host", sorted(over), st, msg))
        assert st == _lib.IRE_ERR_INVALID_INPUT and msg == want, (over, st, msg)
        refused.append(over)

    args, size = (f["device_args"], f["device_size"]) if device else (f["host_args"], f["host_args"])
    for px in inputs:
        e = _Entry(engine, fmt, device, px)
        refuse(e, f["stride"], stride=e.bound - 1)
        if device:          # (the host entries take dense images: they have no pitches)
            refuse(e, f["pitch"], row_pitch=3 * e.w - 1)
            if e.n == 2:
                refuse(e, f["pitch"], image_pitch=3 * e.w * (e.h - 1) + 3 * e.w - 1)
        refuse(e, args, n=0)
        refuse(e, args, n=engine.max_batch + 1)
        refuse(e, size, h=8193)
        refuse(e, size, w=8193)
        for name in ("rgb", "chars") + (("lens",) if f["counted"] else ()):
            refuse(e, args if device else f["host_null"], **{name: None})
    assert len(refused) == 2 * (8 if f["counted"] else 7) + (3 if device else 0)
    # the engine is as usable as before
    e = _Entry(engine, fmt, device, inputs[1])
    st, msg = e.call()
    assert st == _lib.IRE_OK, msg
    assert e.texts() == [f["model"](p) for p in inputs[1]]
