"""The batcher's file jobs (csrc/batcher.hpp: submit_file and the backend's file hooks) under ThreadSanitizer and AddressSanitizer +
UBSan on the CPU, over the host-only stub backend with its decode hook and a status word per job
(tests/native/batcher_files_stress.cpp, batcher_stub.hpp -- test infrastructure): mixed file and
pixel submitters never share a batch, a flagged file in the middle of a batch fails alone, refused and oversized files create no
job, releases while gathering, and the overflow path."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batcher_files_stress.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + [SRC, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    out = []
    for _ in range(3):          # three runs: the interleavings differ
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        out.append(r.stdout + r.stderr)
        assert r.returncode == 0, out[-1][-4000:]
        assert "batcher_files_stress ok" in r.stdout
    return "\n".join(out)


def test_file_jobs_under_thread_sanitizer(tmp_path):
    # IRE_BATCHER_SYSCLOCK_WAITS: gcc 11's libtsan does not intercept pthread_cond_clockwait (batcher.hpp::wait_deadline)
    log = _build_and_run(tmp_path, "bfs_tsan", ["-fsanitize=thread", "-DIRE_BATCHER_SYSCLOCK_WAITS"])
    assert "WARNING: ThreadSanitizer" not in log, log[-4000:]


def test_file_jobs_under_address_sanitizer(tmp_path):
    log = _build_and_run(tmp_path, "bfs_asan", ["-fsanitize=address,undefined"])
    assert "ERROR: AddressSanitizer" not in log and "runtime error" not in log and "LeakSanitizer" not in log, log[-4000:]
