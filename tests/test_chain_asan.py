"""The CPU backend's chain buffers and the denoiser guided through them under AddressSanitizer +
UBSan: `make asan` builds tests/native/chain_asan.cpp (its own main, no Python, no context layer) against the sanitized bdpt_cpu.cpp, and the run -- whole frame, window, two-plane
request on cornell_mirror at 33x9, both branches, then bdpt_cpu_denoise with materials = through,
into buffers of exactly the packed size -- must end with status 0 and without a report."""
import os
import subprocess

from conftest import REPO, SCENES

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")


def test_cpu_render_chain_and_denoise_through_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ASAN, "chain_asan"), DAT, os.path.join(SCENES, "cornell_mirror.scn")], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("mismatches so far 0") == 2 and "denoise through:" in r.stdout
