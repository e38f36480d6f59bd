"""Buffer ownership (csrc/device_buf.hpp) on the CPU box: tests/native/device_buf_test.cpp (test infrastructure; libire.so includes the
same header over hipMalloc / hipHostMalloc) runs Buf, BufSet, the engine's two buffer groups and the batcher slot's staging over a
counting memory policy that can be told to throw on its k-th allocation, once at -O2 and once under ASan + UBSan.

Under IRE_DEBUG_POISON every Buf enters its allocation in csrc/buf_registry.hpp's registry (what ire_debug_poison_scratch walks): the
same program's `registry` mode holds the registry to the live buffers through alloc, free, reset, grow, a failed grow, moves and two
threads, under ASan + UBSan and under ThreadSanitizer.  A source scan holds csrc/ to "every allocation is a Buf of the two policies",
which is what makes the registry complete.

The workspace table and bytes_per_image are compared here with the PARENT's code restated independently: commit 66d745c's
Engine::ensure_workspace loop and its closed-form Engine::bytes_per_image."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "device_buf_test.cpp")
SAN_MARKS = ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer", "ThreadSanitizer")
CSRC = os.path.join(ROOT, "image_restoration_platform_amd", "csrc")
WIDTHS = (32, 64, 128, 256)
SHAPES = [(1, 16, 16), (3, 64, 40), (8, 1024, 1024), (1, 8192, 8192)]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer", "-Wall", "-pthread"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, *args, poison=None):
    env = {k: v for k, v in os.environ.items() if k != "IRE_DEBUG_POISON"}
    if poison is not None:
        env["IRE_DEBUG_POISON"] = poison
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300, env=env)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and not any(m in log for m in SAN_MARKS), log
    return r.stdout


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("device_buf")
    return _build(tmp, "db", ["-O2"]), _build(tmp, "db_asan", ["-O1", "-fsanitize=address,undefined"])


def test_ownership_under_allocation_failure(exes):
    """Buf, BufSet, IoBufs / FuseBufs with every allocation of a regrow failing in turn, batch_room, and the slot's reserve with every
    allocation failing in turn: the program exits 0 and prints ok, optimised and under the sanitizers (no report, no leak)."""
    for exe in exes:
        assert _run(exe) == "ok\n"


def test_registry_follows_every_buffer(exes, tmp_path):
    """IRE_DEBUG_POISON set: an entry per live allocation with its size, kind and use; none after free, reset, a failed grow, a failed
    regrow or reserve, or for a moved-from buffer; two threads allocating at once.  ASan + UBSan, and ThreadSanitizer."""
    tsan = _build(tmp_path, "db_tsan", ["-O1", "-fsanitize=thread"])
    for exe in (exes[0], exes[1], tsan):
        assert _run(exe, "registry", poison="90") == "ok\n"


def test_registry_is_off_without_the_variable(exes):
    """the program's plain mode asserts that nothing entered the registry; the `registry` mode refuses to pass without the variable,
    and a value that is no byte counts as unset"""
    for bad in (None, "", "256", "-1", "x", "0x5A", "+90", " 90", "0090"):
        env = {k: v for k, v in os.environ.items() if k != "IRE_DEBUG_POISON"}
        if bad is not None:
            env["IRE_DEBUG_POISON"] = bad
        r = subprocess.run([exes[0], "registry"], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 1 and "BufRegistry::on()" in r.stderr, (bad, r.stderr)


def _code(path):
    """a source file without its comments"""
    txt = open(path, errors="ignore").read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def test_every_allocation_goes_through_the_two_policies():
    """The registry is complete by construction: in csrc/ only common.hpp's DeviceMem::alloc / PinnedMem::alloc call the allocators, only
    their free calls the deallocators, and every Buf / BufSet (and the three groups made of them) is instantiated over those two."""
    alloc_calls = re.compile(r"\b(hipMalloc\w*|hipHostMalloc|hipHostAlloc|hipExtMallocWithFlags|hipMemPoolCreate|hipHostRegister|hipFree\w*|hipHostFree)\s*\(")
    found, policies = [], set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hpp", ".cpp", ".hip", ".h", ".inc")):
            continue
        code = _code(os.path.join(CSRC, name))
        found += [(name, m.group(1)) for m in alloc_calls.finditer(code)]
        for m in re.finditer(r"\b(?:Buf|BufSet|IoBufs|FuseBufs)<\s*(\w+)\s*>", code):
            policies.add((name if m.group(1) not in ("DeviceMem", "PinnedMem", "Mem") else "", m.group(1)))
        for m in re.finditer(r"\bSlotMem<\s*(\w+)\s*,\s*(\w+)\s*>", code):
            policies.add(("", m.group(1))), policies.add(("", m.group(2)))
    assert sorted(found) == [("common.hpp", "hipFree"), ("common.hpp", "hipFree"), ("common.hpp", "hipHostFree"), ("common.hpp", "hipHostMalloc"), ("common.hpp", "hipMalloc")], found
    # `Mem`, `Dev`, `Pin`: device_buf.hpp's own template parameters
    assert {p for f, p in policies if f == ""} >= {"DeviceMem", "PinnedMem"}
    assert all(f == "device_buf.hpp" and p in ("Dev", "Pin") for f, p in policies if f), policies


def parent_ensure_workspace(n, h, w, lanes):
    """the sizes the parent's Engine::ensure_workspace requests for a fresh shape, in its order"""
    cdiv = lambda a, b: (a + b - 1) // b
    per = cdiv(n, lanes)
    out = []
    for _ in range(lanes):
        for l in range(4):
            b = per * (h >> l) * (w >> l) * WIDTHS[l] * 2
            out += [b] * 4
            if l < 3:
                out.append(b)
        tiles0 = cdiv(h, 4) * cdiv(w, 32)
        out += [per * tiles0 * 16 * 4] * 2
        out.append(per * 256 * 8)
    return out


def parent_bytes_per_image(h, w):
    """the parent's closed form"""
    b = 0
    for l in range(4):
        b += (h >> l) * (w >> l) * WIDTHS[l] * 2 * (4 + (1 if l < 3 else 0))
    b += 2 * ((h + 3) // 4) * ((w + 31) // 32) * 16 * 4 + 256 * 8
    return b + h * w * 3 * 2


def test_workspace_table_equals_the_parents_loop(exes):
    out = _run(exes[0], "dump")
    assert _run(exes[1], "dump") == out
    lines = [ln.split() for ln in out.splitlines()]
    ws = {tuple(map(int, ln[1:5])): [tuple(map(int, e.split(":"))) for e in ln[5:]] for ln in lines if ln[0] == "ws"}
    assert sorted(ws) == sorted((n, h, w, lanes) for n, h, w in SHAPES for lanes in (1, 2, 3))
    # act[l][0..3], skip[l] per level, then stats, stats2, ab: level * 8 + b | 32, 33, 34
    slots = [l * 8 + b for l in range(4) for b in range(5) if not (l == 3 and b == 4)] + [32, 33, 34]
    for (n, h, w, lanes), table in ws.items():
        assert [s for s, _ in table] == slots
        assert [b for _, b in table] * lanes == parent_ensure_workspace(n, h, w, lanes), (n, h, w, lanes)
    bpi = [tuple(map(int, ln[1:])) for ln in lines if ln[0] == "bpi"]
    assert [(h, w) for h, w, _ in bpi] == [(h, w) for _, h, w in SHAPES] + [(16, 16), (24, 4096), (4096, 24)]
    for h, w, b in bpi:
        assert b == parent_bytes_per_image(h, w), (h, w)
    # the partials of one image: 16 floats per 4 x 32 tile of level 0 (what strips.cpp and both workspaces size by)
    assert [ln[1:] for ln in lines if ln[0] == "partials"] == [["64", "160", str(2048 * 256 * 16)]]
