"""The path-pass planner for masked calls (bdpt_plan.h with bdpt_plan_in::ntiles; what
bdpt_path_passes_tiles launches) against figures worked out by hand: tests/native/plan_tiles_check.cpp,
host code only.  `make` builds it beside the other native checks; a tree without the binary
compiles it here."""
import os
import subprocess

from conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"


def test_masked_path_pass_planner(tmp_path):
    exe = os.path.join(REPO, "tests", "native", "plan_tiles_check")
    src = exe + ".cpp"
    deps = [src] + [os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "csrc", h) for h in ("bdpt_plan.h", "bdpt_device.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        exe = str(tmp_path / "plan_tiles_check")
        subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout
