"""The CPU backend's path passes over a tile mask under AddressSanitizer + UBSan: `make asan` builds
tests/native/tiles_asan.cpp (its own main, no Python, no context layer) against the sanitized
bdpt_cpu.cpp -- masks A, B and the empty one at 97x65 and 33x9, in heap buffers of exactly the
mask's size -- and the sanitized C host runs `--until E --adaptive` through the HIP-free context
layer (tests/native/asan_cpu_abi_noise.cpp).  Both must end with status 0 and without a report."""
import os
import re
import subprocess

from conftest import REPO

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")


def _env():
    return dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                UBSAN_OPTIONS="print_stacktrace=1")


def _clean(r):
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])


def test_cpu_masked_path_passes_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    r = subprocess.run([os.path.join(ASAN, "tiles_asan"), DAT], cwd=REPO, env=_env(), capture_output=True, text=True,
                       timeout=600)
    _clean(r)
    assert r.stdout.count("mismatches 0") == 2, r.stdout
    for frame, tiles in (("97x65", "4x9"), ("33x9", "2x2")):
        m = re.search(frame + r": tiles (\S+), pixel-calls rendered (\d+) kept (\d+)", r.stdout)
        assert m and m.group(1) == tiles and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout


def test_smallpt_adaptive_under_asan(tmp_path):
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    scn = os.path.join(REPO, "assets", "scenes", "cornell.scn")
    cmd = [os.path.join(ASAN, "smallpt_asan"), "64", "48", scn, "--device", "-1", "--dat", DAT, "--until", "0.1",
           "--max-spp", "64", "--adaptive", "--batch", "8", "--out", "a.ppm"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    _clean(r)
    m = re.search(r"^Until 0\.1 adaptive: (\d+) passes \((\d+) in this render\), (converged|not converged), "
                  r"(\d+) of 21 tiles left, (\d+) pixel-passes of (\d+) \(width x height x passes\)$", r.stderr, re.M)
    assert m, r.stderr[-2000:]
    passes, pp, whole = int(m.group(1)), int(m.group(5)), int(m.group(6))
    assert 8 <= passes <= 64 and whole == 65 * 49 * passes and 0 < pp < whole, m.group(0)
    assert os.path.getsize(str(tmp_path / "a.ppm")) > 0
