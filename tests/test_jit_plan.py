"""The build plan of the scene-specialised path kernels (bdpt_jit_plan.h: variants, the environment
as values, scene literals, option strings, first attempt and the verdict on each build) on the
CPU, against figures worked out by hand (tests/native/jit_plan_check.cpp)."""
import os
import subprocess

import pytest

from conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_jit_build_plan(tmp_path):
    exe = tmp_path / "jit_plan_check"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-o", str(exe),
                           os.path.join(REPO, "tests", "native", "jit_plan_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout
