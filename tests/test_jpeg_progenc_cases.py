"""The coefficient cases of tests/jpeg_progenc_cases.py on the CPU: every case raises the events it was built for, the model's file of
it stays inside the bound, and the decoder's model reads the file back to the coefficients given."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_opt_model as opt            # noqa: E402
import jpeg_prog_model as dec           # noqa: E402
import jpeg_progenc_cases as cases      # noqa: E402
import jpeg_progenc_model as model      # noqa: E402


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_fires_its_rule(name):
    h, w, q, s, flat = cases.case(name)
    f, events = cases.want(name)
    for e in cases.BUILDERS[name][1]:
        assert events.get(e, 0) >= 1, (name, e, events)
    assert len(f) <= model.file_bound(h, w, q, s)
    assert (len(f) + 2) // 3 * 4 <= model.base64_bound(h, w, q, s)


def test_what_the_cases_hold():
    h, w, q, s, flat = cases.case("row_of_1024")
    assert model.restart_interval(h, w, s, 1) == 1024
    h, w, q, s, flat = cases.case("dummy_blocks")
    planes = model.planes_from_flat(flat, h, w, s)
    geo, _ = model.geometry(h, w, s)
    assert geo[0][:2] == (4, 2) and geo[0][2:] == (3, 1)
    assert np.array_equal(planes[0][:3, 1, 0], planes[0][:3, 0, 0]) and planes[0][3, 0, 0] == planes[0][2, 1, 0] == planes[0][3, 1, 0]      # the dummy DCs
    assert planes[0][:3, 0, 0].any() and not planes[0][:, 1, 1:].any() and not planes[0][3, :, 1:].any()
    h, w, q, s, flat = cases.case("early_flush")
    assert np.abs(flat[:, 1:]).min() >= 4 and model.geometry(h, w, s)[0][0][3] >= 16
    for name in ("extreme_444", "extreme_420"):
        h, w, q, s, flat = cases.case(name)
        assert q == 100 and np.abs(flat[:, 1:]).max() == 1020 and flat[:, 0].min() == -1024 and flat[:, 0].max() == 1016


# (row_of_1024 is left out for its run time alone: the decoder's model walks its 3072 blocks bit by bit, some 20 s; the encoder's
# model, the CPU program and the device all take the case)
@pytest.mark.parametrize("name", [n for n in cases.NAMES if n != "row_of_1024"])
def test_the_decoder_model_reads_every_case_back(name):
    h, w, q, s, flat = cases.case(name)
    planes = model.planes_from_flat(flat, h, w, s)
    grids = dec.coefficients(dec.plan(cases.want(name)[0]))
    geo, _ = model.geometry(h, w, s)
    for c in range(3):
        own = grids[c][..., opt.ZIGZAG]
        if c == 0 and s == 2:       # the AC of a dummy block is never sent; its DC is
            assert np.array_equal(own[:, :, 0], planes[c][:, :, 0]) and np.array_equal(own[:geo[0][2], :geo[0][3]], planes[c][:geo[0][2], :geo[0][3]]), name
        else:
            assert np.array_equal(own, planes[c]), (name, c)
