"""The inputs of tests/test_fusion_align_gpu.py have the properties those tests rely on -- shown with the oracle alone (CPU):
a case that does not make its candidate win, does not tie, or no longer reaches its launch shape would test nothing on the GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_cases as fc      # noqa: E402
from oracle import fusion as ofu      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_COARSE = {(a, b) for a in range(-4, 5) for b in range(-4, 5)}
ALL_FINE = {(a, b) for a in range(-3, 4) for b in range(-3, 4)}


def test_geometry_constants_are_those_of_the_kernel_source():
    src = open(os.path.join(ROOT, "image_restoration_platform_amd", "csrc", "fusion.hip")).read()

    def pair(name):
        m = re.search(r"\b%s = MODE == 0 \? (\d+) : (\d+);" % name, src)
        assert m, name
        return int(m.group(1)), int(m.group(2))
    assert pair("TW") == fc.TW and pair("SR") == fc.SR
    assert (fc.CR, fc.FR, fc.FM) == tuple(int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("CR", "FR", "FM"))
    assert int(re.search(r"constexpr int FUSE_SAD_GRID = (\d+);", src).group(1)) == fc.SAD_GRID
    assert 256 * int(re.search(r"#define FUSE_FL (\d+)", src).group(1)) == fc.ROWSUM_PASS
    assert "std::max(32, 512 / ((k - 1) * nsets))" in src                     # the default cap geometry() restates
    assert "h > %d || w > %d" % (fc.MAX_DIM, fc.MAX_DIM) in src
    assert fc.geometry(1024, 1024)["fine"]["G"] == 124 and fc.geometry(1024, 1024, k=3, nsets=8)["coarse"]["G"] == 32   # fuse_launch's notes


def test_decompose_is_the_oracles_alignment():
    rng = np.random.default_rng(1)
    for views in (fc.cover_views(5, 3)[0], fc.uncorrelated(9, 3, 64, 72), rng.integers(0, 256, (2, 96, 64, 3), dtype=np.uint8)):
        d = fc.decompose(views)
        sh = ofu.align(views)
        assert len(d) == len(views) - 1
        for v, (c, f, ct, ft) in enumerate(d, start=1):
            assert (4 * c[0] + f[0], 4 * c[1] + f[1]) == tuple(sh[v])
            assert ct.shape == (9, 9) and ft.shape == (7, 7)
            assert ct[c[0] + 4, c[1] + 4] == ct.min() and ft[f[0] + 3, f[1] + 3] == ft.min()


@pytest.mark.parametrize("k", [2, 3])
def test_cover_makes_every_candidate_win_and_recovers_every_shift(k):
    assert len(fc.COVER) == len(fc.COVER3_VIEW2) and len(set(fc.COVER)) == len(fc.COVER) <= 150
    assert sorted(i for b in fc.cover_batches() for i in b) == list(range(len(fc.COVER))) and max(map(len, fc.cover_batches())) <= 16
    coarse = [set() for _ in range(k - 1)]
    fine = [set() for _ in range(k - 1)]
    for i in range(len(fc.COVER)):
        views, planted = fc.cover_views(i, k)
        d = fc.decompose(views)
        for v, (c, f, _, _) in enumerate(d):
            assert (4 * c[0] + f[0], 4 * c[1] + f[1]) == tuple(planted[v + 1]), (i, v)
            coarse[v].add(c)
            fine[v].add(f)
    for v in range(k - 1):            # every view's search on its own: a wave of the argmin per view
        assert coarse[v] == ALL_COARSE, (v, sorted(ALL_COARSE - coarse[v]))
        assert fine[v] == ALL_FINE, (v, sorted(ALL_FINE - fine[v]))


def test_tie_cases_tie_and_the_named_candidate_wins():
    cases = fc.tie_cases()
    deciders = set()
    for name, (views, want) in cases.items():
        assert views.dtype == np.uint8 and len(want) == len(views) - 1, name
        d = fc.decompose(views)
        for v, ((c, f, ct, ft), (shift, table, n)) in enumerate(zip(d, want)):
            assert (4 * c[0] + f[0], 4 * c[1] + f[1]) == shift, (name, v, c, f)
            t, win, r = (ct, c, 4) if table == "coarse" else (ft, f, 3)
            at_min = [(a - r, b - r) for a, b in zip(*np.nonzero(t == t.min()))]
            assert len(at_min) == n >= 2 and win in at_min, (name, v, at_min)
            man = [abs(a) + abs(b) for a, b in at_min]
            by_man = [s for s, m in zip(at_min, man) if m == min(man)]
            deciders.add("manhattan" if len(by_man) == 1 else "order" if len(set(man)) == 1 else "both")
            assert win == min(by_man), (name, v)
            assert win != (0, 0) or table == "coarse", name                    # a tie among non-zero candidates
            if table == "fine":
                assert ft.min() == 0                                           # the rolled view matches exactly
    assert deciders == {"manhattan", "order", "both"}
    assert {len(v) for v, _ in cases.values()} == {2, 3}
    assert any(w[0][1] == "coarse" for _, w in cases.values())


def test_uncorrelated_views_have_small_margins_and_distinct_shapes():
    shapes = [(h, w) for _, _, h, w in fc.UNCORRELATED]
    assert len(set(shapes)) == len(shapes) and {k for _, k, _, _ in fc.UNCORRELATED} == {2, 3}
    assert len({s for s, _, _, _ in fc.UNCORRELATED}) == len(fc.UNCORRELATED)
    multi = 0
    for seed, k, h, w in fc.UNCORRELATED:
        g = fc.geometry(h, w, k)
        multi += g["coarse"]["tiles_x"] * g["coarse"]["tiles_y"] > 1 and g["fine"]["tiles_x"] * g["fine"]["tiles_y"] > 1
        for c, f, ct, ft in fc.decompose(fc.uncorrelated(seed, k, h, w)):
            # A SAD over n independent samples scatters by about 0.7 / sqrt(n) of its mean (|a - b| of two uniform bytes: mean 85,
            # sigma 60); a planted shift wins by half the mean.  The runner-up within two such sigmas of the winner: no margin.
            for t, n in ((ct, (h // 4 - 8) * (w // 4 - 8)), (ft, (h - 40) * (w - 40) // 4)):
                lo = np.sort(t.ravel())
                assert lo[1] <= lo[0] * (1 + 1.4 / np.sqrt(n)), (seed, lo[:2], n)
    assert multi >= 4


def test_shapes_reach_the_launch_shapes_they_are_named_for():
    assert {(h, w) for h, w, _, _ in fc.SHAPES.values()} >= {(2048, 64), (64, 2048), (64, 1064), (64, 8192), (8192, 64), (64, 72),
                                                            (104, 64), (112, 64)}
    for name, (h, w, shifts, claims) in fc.SHAPES.items():
        assert h % 8 == 0 and w % 8 == 0 and 64 <= h <= fc.MAX_DIM and 64 <= w <= fc.MAX_DIM
        g = fc.geometry(h, w, k=3)
        assert claims
        for (search, key), value in claims.items():
            assert g[search][key] == value, (name, search, key, g[search][key])
    # the row sum of the last workgroup runs more than one pass at the default cap
    g = fc.geometry(2048, 64, k=3)
    assert 2 * g["coarse"]["G"] * fc.NC > fc.ROWSUM_PASS and 2 * g["fine"]["G"] * fc.NF > fc.ROWSUM_PASS
    assert any(fc.geometry(h, w, k=3)[s]["rowsum_passes"] > 1 for h, w, _, _ in fc.SHAPES.values() for s in ("coarse", "fine"))


@pytest.mark.parametrize("name", sorted(fc.SHAPES))
def test_shapes_plant_a_negative_coarse_shift_on_the_long_axis(name):
    h, w, shifts, _ = fc.SHAPES[name]
    axis = 0 if h > w else 1
    d = fc.decompose(fc.shape_views(name, 3))
    for v, (c, f, _, _) in enumerate(d):
        assert (4 * c[0] + f[0], 4 * c[1] + f[1]) == shifts[v], (name, v)         # the oracle recovers what was planted
    assert d[0][0][axis] < 0, (name, d[0][0])                                      # view 1 of both k = 2 and k = 3
