"""The CPU backend's sphere-following history under AddressSanitizer + UBSan: `make asan` builds
tests/native/follow_asan.cpp (its own main, no Python, no context layer) against the sanitized
bdpt_cpu.cpp, and the run -- a 7x5 and a 40x33 frame; one ball, the last sphere, both and a wall
moved; the emitter moved, a radius changed and a sphere fewer as the refused scenes -- must end
with status 0 and without a report.  Nothing is preloaded.  The sanitized smallpt is run through
--reproject-follow besides."""
import os
import re
import subprocess

from conftest import REPO, SCENES

ASAN = os.path.join(REPO, "tests", "native", "_asan")
DAT = os.path.join(REPO, "assets", "data", "MersenneTwister.dat")
ENV = dict(BDPT_CPU_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _clean(r):
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])


def test_cpu_follow_under_asan():
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, **ENV)
    r = subprocess.run([os.path.join(ASAN, "follow_asan"), DAT], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    _clean(r)
    for frame in ("7x5", "40x33"):
        m = re.search(frame + r": followed (\d+), through the last entry (\d+), mismatches (\d+)", r.stdout)
        assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0 and int(m.group(3)) == 0, r.stdout
        assert len(re.findall(frame + r" [^:]+: state 2,", r.stdout)) == 4, r.stdout
        assert len(re.findall(frame + r" [^:]+: state 3, moved-sphere pixels with history 0,", r.stdout)) == 3, r.stdout


def test_the_sanitized_host_accepts_reproject_follow(tmp_path):
    subprocess.check_call(["make", "-s", "-j4", "asan"], cwd=REPO, timeout=600)
    env = dict(os.environ, **ENV)
    out = str(tmp_path / "x.ppm")
    scn = os.path.join(SCENES, "cornell_diff.scn")
    cmd = [os.path.join(ASAN, "smallpt_asan"), "20", "19", scn, "--spp", "2", "--keys", "++6a4-", "--device", "-1",
           "--dat", DAT, "--reproject", "--reproject-follow", "--out", out]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    _clean(r)
    assert "failed" not in r.stderr, r.stderr[-2000:]
    want = str(tmp_path / "want.ppm")
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    subprocess.run([exe] + cmd[1:-1] + [want], check=True, cwd=REPO, capture_output=True, timeout=120)
    assert open(out, "rb").read() == open(want, "rb").read()   # and writes the product's file
