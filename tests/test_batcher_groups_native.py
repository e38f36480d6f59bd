"""The batcher's fusion jobs (csrc/batcher.hpp: submit_group, slots of max_batch / k jobs, the backend's launch under a Group key) under
ThreadSanitizer and AddressSanitizer + UBSan on the CPU box, over the host-only stub backend (tests/native/batcher_groups_stress.cpp, batcher_stub.hpp),
exactly as tests/test_batcher_native.py runs the pixel jobs' state machine."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batcher_groups_stress.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + [SRC, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = []
    for _ in range(3):          # three runs: the interleavings differ
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        out.append(r.stdout + r.stderr)
        assert r.returncode == 0, out[-1][-4000:]
        assert "batcher_groups_stress ok" in r.stdout
    return "\n".join(out)


def test_fusion_jobs_state_machine_under_thread_sanitizer(tmp_path):
    # IRE_BATCHER_SYSCLOCK_WAITS: gcc 11's libtsan does not intercept pthread_cond_clockwait (batcher.hpp::wait_deadline)
    log = _build_and_run(tmp_path, "bg_tsan", ["-fsanitize=thread", "-DIRE_BATCHER_SYSCLOCK_WAITS"])
    assert "WARNING: ThreadSanitizer" not in log, log[-4000:]


def test_fusion_jobs_state_machine_under_address_sanitizer(tmp_path):
    log = _build_and_run(tmp_path, "bg_asan", ["-fsanitize=address,undefined"])
    assert "ERROR: AddressSanitizer" not in log and "runtime error" not in log and "LeakSanitizer" not in log, log[-4000:]
