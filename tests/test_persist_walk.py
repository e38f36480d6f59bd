"""The work cursor of the persistent conv kernels (csrc/persist.hpp) on the CPU: tests/native/persist_walk.cpp compiles the header the
kernels include with plain g++ and prints what every workgroup's cursor hands out, forward and reverse; this file decodes the same
walk from scratch (a division decode of L = lo + jx + k * nwx, restated here from the header's opening comment) and compares.

Geometries (tiles_x, tiles_y, nimg, nblocks, nkc) x grid sizes G: a single item; items < G; a prime-sized grid of tiles; an eighth that
is exactly one image ((32, 64, 8, 1, 1) at G = 256: the flagship's level 0); strides that carry through every digit; G < 8 (fewer XCD
groups than XCDs) and G = 12 (groups of unequal size)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "persist_walk.cpp")
SAN_MARKS = ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer")
GEOS = [(1, 1, 1, 1, 1), (3, 2, 3, 2, 4), (11, 13, 3, 1, 2), (32, 64, 8, 1, 1), (4, 8, 8, 2, 16), (2, 1, 5, 4, 8), (5, 3, 2, 3, 1), (64, 32, 1, 2, 2)]
GRIDS = [1, 3, 8, 12, 256, 5, 512]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    log = r.stdout[-500:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and not any(m in log for m in SAN_MARKS), log
    return r.stdout


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("persist_walk")
    out = _run(_build(tmp, "pw", ["-O2"]))
    out_san = _run(_build(tmp, "pw_san", ["-O1", "-fsanitize=address,undefined"]))
    assert out_san == out                          # under ASan + UBSan: the same lines, no report
    table = {}
    for ln in out.splitlines():
        head, stages, past = ln.split("|")
        h = tuple(int(v) for v in head.split())
        assert h[:8] not in table
        table[h[:8]] = (h[8:], [tuple(int(v) for v in s.split(",")) for s in stages.split()], [tuple(int(v) for v in s.split(",")) for s in past.split()])
    return table


def decode(geo, G, block):
    """the items of workgroup `block`, ascending, each (img, ty, tx, nb, tile): divisions only"""
    tiles_x, tiles_y, nimg, nblocks, _ = geo
    per_img = tiles_x * tiles_y
    items = per_img * nimg * nblocks
    X = min(G, 8)
    xcd, jx = block % X, block // X
    nwx = (G - xcd + X - 1) // X
    lo, hi = items * xcd // X, items * (xcd + 1) // X
    out = []
    for L in range(lo + jx, hi, nwx):
        nb, t = L % nblocks, L // nblocks
        img, tile = t // per_img, t % per_img
        out.append((L, (img, tile // tiles_x, tile % tiles_x, nb, tile)))
    return out


def test_the_dump_covers_every_case(walks):
    assert set(walks) == {g + (G, rev, b) for g in GEOS for G in GRIDS for rev in (0, 1) for b in range(G)}


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "x".join(map(str, g)))
def test_walks(walks, geo):
    nkc = geo[4]
    n_all = geo[0] * geo[1] * geo[2] * geo[3]
    for G in GRIDS:
        seen = []
        idle = 0
        for b in range(G):
            want = decode(geo, G, b)
            items = [it for _, it in want]
            (fS, fn, ffirst, flast), fwd, fpast = walks[geo + (G, 0, b)]
            (rS, rn, rfirst, rlast), rev, rpast = walks[geo + (G, 1, b)]
            # forward: today's walk, the from-scratch decode with kc counting up inside every item
            assert fwd == [it + (kc,) for it in items for kc in range(nkc)], (G, b)
            # reverse: the same items last item first, kc still ascending
            assert rev == [it + (kc,) for it in reversed(items) for kc in range(nkc)], (G, b)
            # S and my_items: the same in both directions
            assert (fS, fn) == (rS, rn) == (len(items) * nkc, len(items)), (G, b)
            if items:
                lo_img, hi_img = min(it[0] for it in items), max(it[0] for it in items)
                assert (ffirst, flast) == (rfirst, rlast) == (lo_img, hi_img), (G, b)
                # stepped past its last stage the cursor stays on it
                assert fpast == [fwd[-1]] * 3 and rpast == [rev[-1]] * 3, (G, b)
            else:
                idle += 1
            seen += [L for L, _ in want]
        # over all workgroups every item exactly once
        assert sorted(seen) == list(range(n_all)), G
        # fewer items than workgroups: the rest are idle (S == 0, checked above through len(items) == 0)
        assert idle >= max(0, G - n_all), G
        if G < 8:
            assert idle == max(0, G - n_all), G     # one workgroup per group: idle only where its part of the range is empty


def test_idle_workgroups(walks):
    # (1, 1, 1, 1, 1): one item -- at every G exactly one workgroup runs it, in either direction
    for G in GRIDS:
        for rev in (0, 1):
            S = [walks[(1, 1, 1, 1, 1, G, rev, b)][0][0] for b in range(G)]
            assert sorted(S) == [0] * (G - 1) + [1], (G, rev)
    # G = 3 < 8: three XCD groups of one workgroup each, thirds of the range; (2, 1, 5, 4, 8) has 40 items: 13 + 13 + 14
    assert [walks[(2, 1, 5, 4, 8, 3, 1, b)][0][1] for b in range(3)] == [13, 13, 14]
    # the flagship's level 0 (an eighth is one image, 32 workgroups per group, 64 items each): a reverse walk starts at the image's last rows
    (S, n, first, last), rev, _ = walks[(32, 64, 8, 1, 1, 256, 1, 3)]
    assert (S, n, first, last) == (64, 64, 3, 3) and rev[0][:3] == (3, 63, 0) and rev[-1][:3] == (3, 0, 0)
