"""Upload jobs that carry ICC tables, in the batcher (csrc/batcher.hpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU,
over the host-only stub backend (tests/native/batcher_icc_stress.cpp, batcher_stub.hpp -- test infrastructure): the profile is no part
of the slot key, so two uploads of one key with different tables share a slot, and each job's head reaches the backend's decode with
its own tables."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batcher_icc_stress.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + [SRC, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "batcher_icc_stress ok" in r.stdout
    return log


def test_icc_upload_jobs_under_thread_sanitizer(tmp_path):
    # IRE_BATCHER_SYSCLOCK_WAITS: gcc 11's libtsan does not intercept pthread_cond_clockwait (batcher.hpp::wait_deadline)
    log = _build_and_run(tmp_path, "bis_tsan", ["-fsanitize=thread", "-DIRE_BATCHER_SYSCLOCK_WAITS"])
    assert "WARNING: ThreadSanitizer" not in log, log[-4000:]


def test_icc_upload_jobs_under_address_sanitizer(tmp_path):
    log = _build_and_run(tmp_path, "bis_asan", ["-fsanitize=address,undefined"])
    assert "ERROR: AddressSanitizer" not in log and "runtime error" not in log and "LeakSanitizer" not in log, log[-4000:]
