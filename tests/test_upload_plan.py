"""ire_upload_plan on the CPU (pure host, no engine): the EXIF orientation the parser reads equals Pillow's for Pillow-written files
(`MM` blocks) and for a hand-built `II` block, the sizes equal oracle.preprocess.plan, every broken or foreign block reads as
orientation 1 with the file still accepted, and a file ire_decode_jpeg_plan refuses is refused with the same reason."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upload_cases as uc      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import upload_plan_reason      # noqa: E402
from oracle import preprocess as op      # noqa: E402

PX = uc.smooth(97, 131, 1)      # 131 x 97 (w x h)


def _plan(data, max_dim=2048, accept=0):
    plan, why = upload_plan_reason(data, max_dim, accept)
    assert plan is not None, why
    return plan


def _expect(data, orientation, max_dim, h=97, w=131):
    sh, sw, o, oh, ow = _plan(data, max_dim)
    assert (sh, sw, o) == (h, w, orientation)
    want_w, want_h, _ = op.plan(w, h, orientation, max_dim)
    assert (ow, oh) == (want_w, want_h)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_pillow_written_exif(orientation):
    data = uc.encode(PX, orientation=orientation)
    assert b"Exif\0\0MM" in data[:64]
    assert uc.pillow_orientation(data) == orientation
    for max_dim in (2048, 64, 100):
        _expect(data, orientation, max_dim)
    grey = uc.encode(PX[:, :, 0], orientation=orientation)
    _expect(grey, orientation, 64)


@pytest.mark.parametrize("orientation", range(1, 9))
def test_hand_built_little_endian_block(orientation):
    data = uc.encode(PX, app1=uc.exif_block(orientation, le=True))
    assert uc.pillow_orientation(data) == orientation
    _expect(data, orientation, 64)
    data = uc.encode(PX, app1=uc.exif_block(orientation, le=False))
    _expect(data, orientation, 64)


def test_the_tag_behind_other_entries():
    for le in (False, True):
        blk = uc.exif_block(le=le, entries=[(0x0100, 4, 1, 131), (0x010F, 2, 4, 0x61626300), (0x0112, 3, 1, 8), (0x0128, 3, 1, 2)])      # (values that fit their fields: Pillow reads the block too)
        data = uc.encode(PX, app1=blk)
        assert uc.pillow_orientation(data) == 8
        _expect(data, 8, 64)


BROKEN = {
    "no APP1": None,
    "APP1 that is not Exif": b"http://ns.adobe.com/xap/1.0/\0<x/>",
    "type LONG": uc.exif_block(entries=[(0x0112, 4, 1, 6)]),
    "type LONG, II": uc.exif_block(le=True, entries=[(0x0112, 4, 1, 6)]),
    "count 2": uc.exif_block(entries=[(0x0112, 3, 2, 6)]),
    "value 0": uc.exif_block(0),
    "value 9": uc.exif_block(9, le=True),
    "IFD offset beyond the segment": uc.exif_block(6, ifd_off=5000),
    "IFD offset far beyond": uc.exif_block(6, le=True, ifd_off=0xFFFFFFF0),
    "cut inside the TIFF header": uc.exif_block(6, cut=11),
    "cut inside the entry": uc.exif_block(6, cut=6 + 8 + 2 + 7),
    "cut behind the count": uc.exif_block(6, cut=6 + 8 + 2),
    "wrong magic": uc.exif_block(6)[:8] + b"\0\x2b" + uc.exif_block(6)[10:],
}


@pytest.mark.parametrize("name", sorted(BROKEN))
def test_broken_exif_is_orientation_1_and_never_a_refusal(name):
    data = uc.encode(PX, app1=BROKEN[name])
    assert uc.pillow_pixels(data).shape == PX.shape
    _expect(data, 1, 64)
    _expect(data, 1, 2048)


def test_the_first_exif_block_counts():
    data = uc.encode(PX, orientation=3, app1=uc.exif_block(6, le=True))      # the spliced block lies in front of Pillow's
    _expect(data, 6, 64)
    data = uc.encode(PX, orientation=3, app1=BROKEN["APP1 that is not Exif"])      # a foreign APP1 is passed over
    _expect(data, 3, 64)


def test_refusals_keep_the_decode_plans_reason():
    lib = _lib.load()
    prog = uc.encode(PX, orientation=6, progressive=True)
    cut = uc.encode(PX, orientation=6)[:-40]      # truncated scan
    for data in (prog, cut, b"not a jpeg at all"):
        assert lib.ire_decode_jpeg_plan(data, len(data), None, None, None) == _lib.IRE_ERR_INVALID_INPUT
        why = lib.ire_last_error().decode()
        plan, got = upload_plan_reason(data, 64)
        assert plan is None and got == why and why.startswith("invalid: ")
    # with the accept bit the progressive file is planned as the engine that decodes it would plan it
    assert _plan(prog, 64, _lib.IRE_DECODE_ACCEPT_PROGRESSIVE)[:3] == (97, 131, 6)
    plan, why = upload_plan_reason(prog, 64, 2)
    assert plan is None and "accept" in why
    plan, why = upload_plan_reason(uc.encode(PX), 0)
    assert plan is None and why.startswith("invalid")


def test_the_room_rule_is_planned_too():
    """the cut scan is staged in the job's input place of out_h * out_w * 3 bytes: a file that may need more is refused"""
    data = uc.encode(PX, quality=95)
    assert len(data) > 8 * 6 * 3
    plan, why = upload_plan_reason(data, 8)
    assert plan is None and why.startswith("invalid: ") and "larger than its fitted pixels" in why
    out = [ctypes.c_int() for _ in range(5)]
    assert _lib.load().ire_upload_plan(data, len(data), 0, 64, *[ctypes.byref(v) for v in out]) == 0
    assert _lib.load().ire_upload_plan(data, len(data), 0, 64, None, None, None, None, None) == 0
