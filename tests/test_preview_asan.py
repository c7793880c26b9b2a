"""The CPU backend's denoised preview under AddressSanitizer + UBSan: `make asan` builds
tests/native/preview_asan.cpp (its own main, no Python, no context layer) against the sanitized
bdpt_cpu.cpp, and the run -- a 7x5 and a 40x33 frame, levels 0..8 (at 7x5 every off-centre tap is
outside the frame from step 8 on), history weights from 0 to 1e30, with and without a pass in the
accumulation -- must end with status 0 and without a report."""
import os
import re
import subprocess

from conftest import REPO

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")


def test_cpu_preview_denoise_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ASAN, "preview_asan"), DAT], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("mismatches 0") == 2
    for frame in ("7x5", "40x33"):
        m = re.search(frame + r": calls (\d+), holes (\d+), holes filled (\d+)", r.stdout)
        assert m and all(int(v) > 0 for v in m.groups()), r.stdout
