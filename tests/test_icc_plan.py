"""The ICC planner of upload jobs on the CPU, through the C ABI with no engine (ire_icc_plan_profile, ire_icc_plan_file, ire_upload_plan
with IRE_DECODE_ACCEPT_ICC): the kind, the matrix and the curves are the model's entry by entry for every profile the writer makes;
the sRGB profile is the identity; an untagged file, broken chunk sets, truncated profiles and a profile of the wrong colour space are
no profile, never a refusal; A2B0 / CMYK / Lab profiles are refused with a reason."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_cases as cases      # noqa: E402
import icc_model as model      # noqa: E402
import icc_writer as wr      # noqa: E402
import upload_cases as uc      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import icc_plan_file, icc_plan_profile, upload_plan_reason      # noqa: E402


def _same(t, want):
    assert t.kind == want["kind"]
    if want["kind"] in (model.NONE,):
        return
    assert list(t.m) == list(want["m"])
    rows = 1 if want["kind"] == model.GREY or not any(want["m"]) else 3
    got = np.array([list(t.lin[c]) for c in range(3)])
    assert np.array_equal(got[:rows], np.asarray(want["lin"])[:rows])


@pytest.mark.parametrize("name", sorted(cases.rgb_profiles()))
def test_rgb_profiles_give_the_models_tables(name):
    p = cases.rgb_profiles()[name]
    want = model.plan_profile(p, 3)
    assert want["kind"] in (model.MATRIX, model.IDENTITY)
    t, why = icc_plan_profile(p, 3)
    assert why is None
    _same(t, want)
    # the same through a file, in one chunk and in three out of order
    f = cases.stored_file()
    for tagged in (wr.tag(f, p), wr.tag(f, p, 3, (2, 0, 1))):
        t2, why = icc_plan_file(tagged)
        assert why is None
        _same(t2, want)
        assert uc.pillow_pixels(tagged).tobytes() == uc.pillow_pixels(f).tobytes()      # (Pillow still reads the file)
    # an RGB profile in a grey file is no profile
    t3, why = icc_plan_profile(p, 1)
    assert why is None and t3.kind == model.NONE
    t4, why = icc_plan_file(wr.tag(cases.stored_file(grey=True), p))
    assert why is None and t4.kind == model.NONE


@pytest.mark.parametrize("name", sorted(cases.grey_profiles()))
def test_grey_profiles_give_the_models_curve(name):
    p = cases.grey_profiles()[name]
    want = model.plan_profile(p, 1)
    assert want["kind"] in (model.GREY, model.IDENTITY)
    t, why = icc_plan_profile(p, 1)
    assert why is None
    _same(t, want)
    t2, why = icc_plan_file(wr.tag(cases.stored_file(grey=True), p, 2, (1, 0)))
    assert why is None
    _same(t2, want)
    t3, why = icc_plan_file(wr.tag(cases.stored_file(), p))      # a grey profile in a colour file
    assert why is None and t3.kind == model.NONE


def test_kinds():
    P = cases.rgb_profiles()
    assert icc_plan_profile(P["srgb_v2"])[0].kind == icc_plan_profile(P["srgb_v4"])[0].kind == _lib.IRE_ICC_IDENTITY
    assert icc_plan_profile(P["p3_v4"])[0].kind == icc_plan_profile(P["adobe_v2"])[0].kind == _lib.IRE_ICC_MATRIX
    assert icc_plan_profile(P["curv1"])[0].kind == _lib.IRE_ICC_MATRIX      # sRGB colorants, another curve
    assert icc_plan_profile(cases.grey_profiles()["grey22"], 1)[0].kind == _lib.IRE_ICC_GREY
    m = list(icc_plan_profile(P["p3_v4"])[0].m)
    # P3 red is outside sRGB; white stays white as far as the published colorants let it: their X sums differ by 9e-5 (0.96420 against
    # 0.96429), times inv(M_sRGB)'s 3.14 and 16384 is 4.6, and three roundings add 1.5
    assert m[0] > 16384 and m[1] < 0 and abs(sum(m[0:3]) - 16384) <= 7


def test_no_profile_is_never_a_refusal():
    f = cases.stored_file()
    p = cases.rgb_profiles()["p3_v4"]
    ch = wr.chunks(p, 3)
    big = wr.chunks(p + b"\0" * ((1 << 20) + 1 - len(p)), 17)
    sets = {
        "untagged": [],
        "missing chunk": [ch[0], ch[2]],
        "duplicate sequence number": [ch[0], ch[1], ch[1], ch[2]],
        "disagreeing counts": [ch[0], (2, 4, ch[1][2]), ch[2]],
        "sequence number 0": [(0, 3, ch[0][2]), ch[1], ch[2]],
        "count 0": [(1, 0, p)],
        "over 1 MiB": big,
    }
    for name, s in sets.items():
        t, why = icc_plan_file(wr.insert_segments(f, [wr.app2(*c) for c in s]))
        assert why is None and t.kind == _lib.IRE_ICC_NONE, name
    t, why = icc_plan_file(wr.insert_segments(f, [wr.app2(*c) for c in wr.chunks(p + b"\0" * ((1 << 20) - len(p)), 17)]))      # exactly 1 MiB: a profile
    assert why is None and t.kind == _lib.IRE_ICC_MATRIX
    for cut in (0, 1, 127, 131, 132, 200, len(p) - 1):
        t, why = icc_plan_profile(p[:cut] if cut else b"\0", 3)
        assert why is None and t.kind == _lib.IRE_ICC_NONE, cut
    no_sig = p[:36] + b"xxxx" + p[40:]
    assert icc_plan_profile(no_sig)[0].kind == _lib.IRE_ICC_NONE
    outside = bytearray(p)
    outside[128 + 4 + 4:128 + 4 + 8] = (len(p) - 4).to_bytes(4, "big")      # the first tag's offset: its data would leave the profile
    assert icc_plan_profile(bytes(outside))[0].kind == _lib.IRE_ICC_NONE
    missing = wr.assemble([(b"rXYZ", wr.xyz_tag(*wr.SRGB[0])), (b"rTRC", wr.curv())])
    assert icc_plan_profile(missing)[0].kind == _lib.IRE_ICC_NONE


@pytest.mark.parametrize("name", sorted(cases.refused_profiles()))
def test_unsupported_profiles_are_refused_with_a_reason(name):
    p = cases.refused_profiles()[name]
    with pytest.raises(model.Refused):
        model.plan_profile(p, 3)
    t, why = icc_plan_profile(p, 3)
    assert t is None and "invalid: ICC" in why
    f = wr.tag(cases.stored_file(), p)
    t, why = icc_plan_file(f)
    assert t is None and "invalid: ICC" in why
    # the upload plan refuses the file with the same reason when asked to look, and is unchanged when not
    plain = upload_plan_reason(cases.stored_file(), 16, 0)
    assert plain[0] == (24, 40, 6, 10, 6) and plain[1] is None
    assert upload_plan_reason(f, 16, 0) == plain
    assert upload_plan_reason(f, 16, _lib.IRE_DECODE_ACCEPT_ICC) == (None, why)
    assert upload_plan_reason(cases.stored_file(), 16, _lib.IRE_DECODE_ACCEPT_ICC) == plain
    ok = wr.tag(cases.stored_file(), cases.rgb_profiles()["p3_v4"])
    assert upload_plan_reason(ok, 16, _lib.IRE_DECODE_ACCEPT_ICC) == plain
    assert upload_plan_reason(ok, 16, _lib.IRE_DECODE_ACCEPT_ICC | _lib.IRE_DECODE_ACCEPT_PROGRESSIVE) == plain


def test_refused_curves_and_matrices():
    long_table = wr.matrix_profile(wr.SRGB, wr.curv_table(2.2, 4097))
    para5 = wr.matrix_profile(wr.SRGB, b"para\0\0\0\0" + (5).to_bytes(2, "big") + b"\0\0" + wr.s15f16(2.2) * 7)
    wide = wr.matrix_profile(((3.0, 0.2, 0.0), wr.SRGB[1], wr.SRGB[2]), wr.curv())      # inv(M_sRGB) M has a coefficient beyond 4
    for p in (long_table, para5, wide):
        with pytest.raises(model.Refused):
            model.plan_profile(p, 3)
        t, why = icc_plan_profile(p, 3)
        assert t is None and "invalid: ICC" in why


def test_abi():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.IreIccTransform) == 4 + 36 + 1536
    assert _lib.IRE_FLAG_UPLOAD_ICC == 256 and _lib.IRE_DECODE_ACCEPT_ICC == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ire.h")).read()
    assert "#define IRE_FLAG_UPLOAD_ICC 256u" in header and "#define IRE_DECODE_ACCEPT_ICC 4u" in header
    t = _lib.IreIccTransform()
    assert lib.ire_icc_plan_file(None, 0, ctypes.byref(t)) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_icc_plan_profile(b"x", 1, 2, ctypes.byref(t)) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_icc_to_srgb(None, None, 1, 1, 1, None) == _lib.IRE_ERR_INVALID_INPUT
    for unknown in (2, 8, 2 | 4):
        assert upload_plan_reason(cases.stored_file(), 16, unknown)[0] is None      # unknown accept bits
    # the flag is a known bit of ire_config.flags and no result format; 512 is not known
    import torch
    accepted = _lib.IRE_OK if torch.cuda.is_available() else _lib.IRE_ERR_UNAVAILABLE
    for flags, want in ((256, accepted), (256 | 32 | 8, accepted), (256 | 1 | 4, _lib.IRE_ERR_INVALID_INPUT), (512, _lib.IRE_ERR_INVALID_INPUT)):
        h, cfg = ctypes.c_void_p(), _lib.IreConfig()
        cfg.struct_size, cfg.max_batch, cfg.flags = ctypes.sizeof(_lib.IreConfig), 2, flags
        st = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
        if st == _lib.IRE_OK:
            lib.ire_shutdown(h)
        assert st == want, flags
