"""The JPEG encoder's edge cases without a GPU (tests/jpeg_opt_cases.py): the model equals libjpeg-turbo's file (Pillow) byte for byte on
every case at every setting, so the model can be the device's reference on this content too (tests/test_jpeg_opt_cases_gpu.py); the
conditions the cases exist for hold, counted from the model alone; every file is within the bound; and the size-class rule of
csrc/jpeg.hip's interval kernel (csrc/jpeg_tables.hpp::big_class) is the one restated in Python for all two hundred settings."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_opt_cases as oc      # noqa: E402
import jpeg_opt_model as model   # noqa: E402
from test_jpeg_opt_model import pillow_file      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_equals_libjpeg_turbo_on_every_case_at_every_setting():
    for name, shape in oc.all_cases():
        px = oc.pixels(name, shape)
        for q, s in oc.SETTINGS:
            f, p = oc.encoded(name, shape, q, s)[0], pillow_file(px, q, s)
            first = next((i for i, (a, b) in enumerate(zip(f, p)) if a != b), None)
            assert f == p, (name, shape, q, s, len(f), len(p), first)
            assert len(f) <= model.file_bound(*shape, q, s), (name, shape, q, s)


def test_the_cases_meet_the_conditions_they_exist_for():
    """DC category 11 and AC category 10 in both tables at quality 100, one / two / three ZRL codes in both tables, DC + EOB blocks, a
    last interval of one MCU, an interval without padding and one that ends in a stuffed 0xFF at either sampling; at 4:2:0 dummy blocks
    behind a DC difference of category 10 or more and dummy blocks whose copied DC is neither 0 nor the first block's; the fullest
    interval at least 0.45 of the big class's 9448 raw bytes at quality 100 and 0.35 of the small class's 5034 at its last quality."""
    sm = oc.assert_conditions()
    for key in (0, 2):
        print("sampling %d: %s" % (key, sm[key]))
    for q, s in oc.SETTINGS:
        raw = oc.RAW_BIG if oc.big_class(q, s) else oc.RAW_SMALL
        print("q %3d s %d: the fullest interval %4d raw bytes, %.2f of %d" % (q, s, sm[(q, s)], sm[(q, s)] / raw, raw))
    # every content is in a batch, every batch fits one call of the session's engine, black lies beside cells2
    assert {n for names in oc.BATCHES.values() for n in names} == set(oc.CONTENT) and all(len(v) <= 8 for v in oc.BATCHES.values())
    assert set(oc.BATCHES) == set(oc.SHAPES)
    for names in list(oc.BATCHES.values())[:2]:
        assert abs(names.index("black") - names.index("cells2")) == 1
    # the shapes: MCU counts and the last interval, as the module's head says
    counts = {shape: [((shape[0] + p - 1) // p) * ((shape[1] + p - 1) // p) for p in (8, 16)] for shape in oc.SHAPES}
    assert counts == {(33, 130): [85, 27], (41, 139): [108, 27], (8, 136): [17, 9]}
    assert [c % r for c, r in zip(counts[(8, 136)], (16, 8))] == [1, 1] and 108 % 16 == 12


def test_the_size_class_rule(tmp_path):
    """(R * mcu_bits_max + 7) // 8 <= 5034: monotone in the quality, the last small quality 86 at 4:4:4 (4864 bytes; 87: 5166) and 85 at
    4:2:0 (5034; 86: 5246), and equal to csrc/jpeg_tables.hpp::big_class -- what geom_of calls -- for all two hundred settings."""
    raw = {s: [(model.R_OF[s] * model.mcu_bits_max(q, s) + 7) // 8 for q in range(1, 101)] for s in (0, 2)}
    big = {s: [int(oc.big_class(q, s)) for q in range(1, 101)] for s in (0, 2)}
    for s, last in ((0, 86), (2, 85)):
        assert raw[s] == sorted(raw[s]) and big[s] == sorted(big[s])
        assert big[s] == [0] * last + [1] * (100 - last), (s, big[s])
        assert raw[s][-1] <= oc.RAW_BIG
    assert (raw[0][85], raw[0][86], raw[2][84], raw[2][85]) == (4864, 5166, 5034, 5246)
    assert raw[2][99] == oc.RAW_BIG and raw[2][84] == oc.RAW_SMALL
    exe = str(tmp_path / "jpeg_opt_tables_dump")
    src = os.path.join(ROOT, "tests", "native", "jpeg_opt_tables_dump.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    got = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    assert [int(v) for v in got["raw_classes"].split()] == [oc.RAW_SMALL, oc.RAW_BIG]
    for s in (0, 2):
        assert [int(v) for v in got["big_class s%d" % s].split()] == big[s], s
        assert [int(v) for v in got["raw_bound s%d" % s].split()] == raw[s], s
        assert [int(v) for v in got["fits_a_class s%d" % s].split()] == [1] * 100, s
