"""The CPU backend's denoiser under AddressSanitizer + UBSan: `make asan` builds
tests/native/denoise_asan.cpp (its own main, no Python, no context layer) against the sanitized
bdpt_cpu.cpp, and the run -- a 7x5 and a 33x9 frame, 1, 3 and 8 levels, both material modes, into
buffers of exactly the packed size -- must end with status 0 and without a report."""
import os
import subprocess

from conftest import REPO

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")


def test_cpu_denoise_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ASAN, "denoise_asan"), DAT], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("mismatches 0") == 2
    assert "7x5: filtered pixels" in r.stdout and "33x9: filtered pixels" in r.stdout
