"""The leaf device functions themselves on the GPU (tests/native/leaf_check.hip, built by `make`):
bdpt_sincos_tab with both tables and bdpt_sincos_dp over every input the render path can pass,
against glibc; bdpt_sample_record against its host side; rcp_rn, rcp_sqrt_rn and bdpt_sqrt_rn -- the
wrappers with their range tests -- over every bit pattern of their domains; div_rn_normal on its two
stated domains; and the three forms of the sphere test with the integer keys against the reference's
branchy statement, on dets in (0, 2^-96) and negative denormal dets, which no scene reaches.  Each
check must report the stated number of inputs (counted by its kernels) and 0 mismatches; a control
that drops rcp_rn's range test must report mismatches.  The two programs run once per
session (about 2 s and 0.6 s on an MI355X)."""
import json
import os
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

SINCOS_N = 268_435_457
INPUTS = {
    "sincos_tab": SINCOS_N, "sincos_dp": SINCOS_N,
    "sample_record": 2 ** 24 + 7 ** 5,
    "rcp_rn": 2 ** 32, "rcp_sqrt_rn": 2 ** 31 + 2 ** 23, "sqrt_rn": 2 ** 31 + 2 ** 23,
    "div_refraction": (2 ** 24 + 1 + 4) * 1024,
    "div_nee": 481 ** 2 + 2 ** 28,
}
SPHERE = ("sphere_isect", "sphere_roots", "sphere_keys")


def run(name):
    exe = os.path.join(REPO, "tests", "native", name)
    assert os.path.exists(exe), f"{exe} is not built (make)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    recs = {}
    for line in out.stdout.splitlines():
        print(line)
        if line.startswith("{"):
            r = json.loads(line)
            recs[r["check"]] = r
    assert out.returncode in (0, 1), (out.returncode, out.stderr[-500:])
    return recs, out.returncode


@pytest.fixture(scope="module")
def leaf(gpu):
    return run("leaf_check")


@pytest.mark.parametrize("check", sorted(INPUTS))
def test_leaf_function_is_exact(leaf, check):
    recs, rc = leaf
    r = recs[check]
    assert r["inputs"] == INPUTS[check], r
    assert r["mismatches"] == 0, r


@pytest.mark.parametrize("check", SPHERE)
def test_sphere_test_equals_the_reference_statement(leaf, check):
    recs, rc = leaf
    r, inp = recs[check], recs["sphere_inputs"]
    assert r["mismatches"] == 0, r
    assert r["inputs"] == inp["tiny_det_cases"] + inp["neg_denormal_cases"] + inp["seeded"]
    # the crafted cases are what they claim, and the seeded ones both hit and miss
    assert inp["tiny_det"] >= 900_000 and inp["neg_denormal_det"] == inp["neg_denormal_cases"] == 511 * 5
    assert inp["seeded"] == 2 ** 24 and inp["seeded"] // 10 < inp["hits"] < inp["seeded"]


def test_every_check_ran_and_the_program_agrees(leaf):
    recs, rc = leaf
    assert set(recs) == set(INPUTS) | set(SPHERE) | {"sphere_inputs", "control_rcp_inrange", "total"}
    assert rc == 0 and recs["total"]["failed"] == 0
    # the control: the reciprocal without its range test must be caught outside [2^-125, 2^125)
    assert recs["control_rcp_inrange"]["inputs"] == 2 ** 32 and recs["control_rcp_inrange"]["mismatches"] > 1_000_000
    print("leaf_check:", recs["total"]["seconds"], "s")


def test_coarse_table_is_exact(gpu):
    recs, rc = run("leaf_check_coarse")
    r = recs["sincos_tab_coarse"]
    assert r["inputs"] == SINCOS_N and r["mismatches"] == 0, r
    assert rc == 0 and recs["total"]["failed"] == 0
