"""The CPU backend's noise-guided denoiser under AddressSanitizer + UBSan: `make asan` builds
tests/native/denoise_noise_asan.cpp (its own main, no Python, no context layer) against the sanitized
bdpt_cpu.cpp, and the run -- a 33x9 and a 7x5 frame, every output into a buffer of exactly its packed
size, eight levels whose steps reach far outside both frames, counters and marks on both sides of
the validity rule and near 2^32 -- must end with status 0 and without a report.  The program runs as
a child process of its own; nothing is preloaded."""
import os
import re
import subprocess

from conftest import REPO

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")


def test_cpu_denoise_noise_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ASAN, "denoise_noise_asan"), DAT], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.count("mismatches 0") == 2
    for frame in ("33x9", "7x5"):
        m = re.search(frame + r": rendered estimates (\d+), uploaded valid (\d+) estimates (\d+)", r.stdout)
        assert m and all(int(v) > 0 for v in m.groups()), r.stdout


def test_smallpt_denoise_noise_under_asan(tmp_path):
    """The sanitized C host through its HIP-free context layer (tests/native/asan_cpu_abi_denoise_noise.cpp):
    --until with --denoise-noise, at the start and after a camera key."""
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    scn = os.path.join(REPO, "assets", "scenes", "cornell.scn")
    cmd = [os.path.join(ASAN, "smallpt_asan"), "32", "24", scn, "--device", "-1", "--dat", DAT, "--until", "0.05",
           "--max-spp", "16", "--batch", "4", "--keys", "a", "--denoise-noise", "0.5", "--out", "u.ppm"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(re.findall(r"^Until 0\.05: \d+ passes", r.stderr, re.M)) == 2, r.stderr[-2000:]
    assert os.path.getsize(str(tmp_path / "u.ppm")) > 0
