"""The decoder's model (tests/jpeg_decode_model.py) against libjpeg-turbo: its pixels equal Pillow's on every case, and its plan
refuses what the device does not decode, each with the right reason.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as model      # noqa: E402


def _check(files):
    for name, data in files.items():
        want = cases.pillow_pixels(data)
        got = model.decode(data)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


def test_model_equals_pillow_on_sizes_samplings_qualities_and_table_variants():
    files = cases.grid_cases()
    samplings = {model.plan(f).sampling for f in files.values()}
    assert samplings == {0, 1, 2, 3}
    assert any(model.plan(f).restart == 3 for f in files.values())
    _check(files)


def test_model_equals_pillow_on_every_partial_mcu_shape():
    files = cases.sweep_cases()
    assert len(files) == 19 * 31
    _check(files)


def test_model_decodes_the_encoders_own_files():
    files = cases.encoder_cases()
    p = model.plan(files["enc_rst_wraps"])
    assert p.restart == 16 and p.nstreams == 12          # RST0..RST7, RST0..RST2
    _check(files)


@pytest.mark.parametrize("name", ["progressive", "cmyk", "420_width4", "cut_in_header"])
def test_plan_refuses_with_the_reason(name):
    data, word = cases.refused_cases()[name]
    with pytest.raises(model.Refused) as e:
        model.plan(data)
    assert word in e.value.reason


def test_where_the_range_limit_stops_being_libjpeg_turbos():
    """inside -512..511 the model's (libjpeg's C) range limit equals Pillow's SIMD code; outside the model refuses to choose"""
    for name, (data, in_range) in cases.out_of_range_cases().items():
        if in_range:
            assert np.array_equal(model.decode(data), cases.pillow_pixels(data)), name
        else:
            with pytest.raises(model.Corrupt):
                model.decode(data)
