"""The CPU backend's noise estimate under AddressSanitizer + UBSan: `make asan` builds
tests/native/noise_asan.cpp (its own main, no Python, no context layer) against the sanitized
bdpt_cpu.cpp, and the run -- a 33x9 and a 7x5 frame, estimates into buffers of exactly the packed
size, counters and marks on both sides of every rule and near 2^32 -- must end with status 0 and
without a report."""
import os
import re
import subprocess

from conftest import REPO

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")


def test_cpu_noise_estimate_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ASAN, "noise_asan"), DAT], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("mismatches 0") == 2
    for frame, tiles, pixels in (("33x9", "2x2", 33 * 9), ("7x5", "1x1", 7 * 5)):
        m = re.search(frame + r": tiles (\S+), rendered valid (\d+), uploaded valid (\d+) pending (\d+) "
                      r"took the mark (\d+)", r.stdout)
        assert m and m.group(1) == tiles and int(m.group(2)) == pixels, r.stdout
        assert all(int(v) > 0 for v in m.groups()[2:]), r.stdout


def test_smallpt_until_under_asan(tmp_path):
    """The sanitized C host through its HIP-free context layer (tests/native/asan_cpu_abi.cpp):
    --until at the start and after a camera and a sphere key, whose re-initialisation clears the mark."""
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    scn = os.path.join(REPO, "assets", "scenes", "cornell.scn")
    cmd = [os.path.join(ASAN, "smallpt_asan"), "32", "24", scn, "--device", "-1", "--dat", DAT, "--until", "0.05",
           "--max-spp", "16", "--batch", "4", "--keys", "a4", "--out", "u.ppm"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r"^Until 0\.05: (\d+) passes \((\d+) in this render\), not converged, worst tile (\S+), mean (\S+)$",
                       r.stderr, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(16, 16), (17, 16), (16, 16)], r.stderr[-2000:]
    # after the camera key the checks fall at 5, 9, 13 and 17 passes: marks at 5 and 13, and 4 fresh
    # samples are fewer than half of 13, so the last check has no valid pixel and reports zeros
    for k, (_, _, w, m) in enumerate(lines):
        assert (float(w) == 0 and float(m) == 0) if k == 1 else (float(w) > 0.05 and float(m) > 0), lines
    assert os.path.getsize(str(tmp_path / "u.ppm")) > 0
