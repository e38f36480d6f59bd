"""The profiles and tagged files the upload-ICC tests share.  Test infrastructure."""
import functools

import numpy as np

import icc_writer as wr
import upload_cases as uc


@functools.lru_cache(maxsize=None)
def rgb_profiles():
    """{name: bytes} of every matrix/TRC profile the writer makes: the three colour spaces, v2 and v4, every curve form"""
    p = {}
    for v in (2, 4):
        p["p3_v%d" % v] = wr.display_p3(v)
        p["adobe_v%d" % v] = wr.adobe_rgb(v)
        p["srgb_v%d" % v] = wr.srgb(v)
    p["para0"] = wr.matrix_profile(wr.ADOBE_RGB, wr.para(0, 2.2), 4)
    p["para1"] = wr.matrix_profile(wr.DISPLAY_P3, wr.para(1, 2.2, 0.95, 0.05), 4)
    p["para2"] = wr.matrix_profile(wr.DISPLAY_P3, wr.para(2, 2.0, 0.9, 0.05, 0.02), 4)
    p["para3"] = wr.matrix_profile(wr.ADOBE_RGB, wr.para(3, *wr.SRGB_PARA3), 4)
    p["para4"] = wr.matrix_profile(wr.DISPLAY_P3, wr.para(4, 2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045, 0.0, 0.0), 4)
    p["curv0"] = wr.matrix_profile(wr.DISPLAY_P3, wr.curv(), 2)
    p["curv1"] = wr.matrix_profile(wr.SRGB, wr.curv_gamma(2.2), 2)
    p["table18"] = wr.matrix_profile(wr.ADOBE_RGB, wr.curv_table(1.8, 1024), 2)
    p["table_short"] = wr.matrix_profile(wr.DISPLAY_P3, wr.curv_table(2.2, 2), 2)
    p["three_curves"] = wr.matrix_profile(wr.DISPLAY_P3, (wr.curv_gamma(1.8), wr.para(0, 2.2), wr.curv_table(2.4, 4096)), 4)
    return p


@functools.lru_cache(maxsize=None)
def grey_profiles():
    return {"grey22": wr.grey_profile(wr.curv_gamma(2.2)), "grey_para": wr.grey_profile(wr.para(3, *wr.SRGB_PARA3), 4),
            "grey_table": wr.grey_profile(wr.curv_table(1.8, 256)), "grey_linear": wr.grey_profile(wr.curv())}


@functools.lru_cache(maxsize=None)
def refused_profiles():
    return {"a2b0": wr.a2b0_profile(), "cmyk": wr.cmyk_profile(), "lab": wr.lab_pcs_profile()}


@functools.lru_cache(maxsize=None)
def stored_file(seed=3, w=40, h=24, orientation=6, progressive=False, grey=False):
    """a small JPEG upload of colour ramps, stored w x h: saturated enough for the conversion to show, smooth enough for its scan to
    be smaller than its pixels fitted inside 16 (the room rule of upload jobs)"""
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([30 + 5 * x + seed, 220 - 6 * y, 60 + 2 * x + 4 * y + seed], -1).clip(0, 255).astype(np.uint8)
    return uc.encode(px[:, :, 0] if grey else px, 60, 0, orientation, progressive)
