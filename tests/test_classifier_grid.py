"""The launch geometry of the classifier scan (csrc/classifier_grid.hpp) on the CPU: tests/native/classifier_grid_dump.cpp compiles the
header classifier.hip includes with plain g++ (once at -O2, once under ASan + UBSan: the same lines) and prints the rule for every
batch size 1..64 and every tile count an image of at most 8192 x 8192 can have.  Checked here: a workgroup count within 1..ntiles,
n * per_img within the rows of the `parts` buffer, balancing that never adds a round, and agreement with the restatement the GPU tests
use to assert which geometry class a case is in (tests/classifier_cases.py::classifier_grid)."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classifier_cases as cc      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "classifier_grid_dump.cpp")
SAN_MARKS = ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer")
MAX_SIDE = 8192


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
def dump(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("classifier_grid")
    out = _run(_build(tmp, "cg", ["-O2"]))
    out_san = _run(_build(tmp, "cg_san", ["-O1", "-fsanitize=address,undefined"]))
    assert out_san == out                          # under ASan + UBSan: the same lines, no report
    consts, tiles, grid = None, {}, {}
    for ln in out.splitlines():
        f = ln.split()
        v = [int(x) for x in f[1:]]
        if f[0] == "C":
            consts = tuple(v)
        elif f[0] == "T":
            assert v[0] not in tiles
            tiles[v[0]] = (v[1], v[2])
        else:
            assert f[0] == "G" and (v[0], v[1]) not in grid
            grid[(v[0], v[1])] = v[2]
    return consts, tiles, grid


def test_constants_and_tile_counts(dump):
    consts, tiles, _ = dump
    assert consts == (cc.CT_H, cc.CT_W, cc.CLS_MAX_WG, cc.CLS_TICKET_CAP) == (16, 256, 768, 64)
    assert sorted(tiles) == list(range(1, MAX_SIDE + 1))
    for v, (tx, ty) in tiles.items():
        # the smallest counts that cover v pixels
        assert (tx - 1) * cc.CT_W < v <= tx * cc.CT_W and (ty - 1) * cc.CT_H < v <= ty * cc.CT_H, v
        assert cc.classifier_grid(1, v, v)[:2] == (tx, ty), v


def test_the_dump_covers_every_batch_and_tile_count(dump):
    consts, tiles, grid = dump
    tx_max, ty_max = tiles[MAX_SIDE]
    counts = {tx * ty for tx in range(1, tx_max + 1) for ty in range(1, ty_max + 1)}
    assert set(grid) == {(n, nt) for n in range(1, consts[3] + 1) for nt in counts}


def test_grid_rule_properties_and_restatement(dump):
    _, _, grid = dump
    for (n, nt), per in grid.items():
        assert 1 <= per <= nt, (n, nt, per)
        assert n * per <= cc.CLS_MAX_WG, (n, nt, per)                     # the rows of `parts`
        cap = min(nt, cc.CLS_MAX_WG // n)
        rounds = -(-nt // per)
        assert rounds == -(-nt // cap), (n, nt, per)                      # balancing never adds a round
        # the restatement, through a shape with that many tiles (one tile column: nt <= 512, else the widest image's 32 columns)
        tx = 1 if nt <= 512 else next(c for c in range(32, 0, -1) if nt % c == 0 and nt // c <= 512)
        h, w = (nt // tx) * cc.CT_H, tx * cc.CT_W
        assert cc.classifier_grid(n, h, w) == (tx, nt // tx, per, rounds, nt // per), (n, nt)
        # tiles_of_last_workgroup: workgroup per - 1 walks per - 1, 2 per - 1, ... below nt
        assert len(range(per - 1, nt, per)) == nt // per
