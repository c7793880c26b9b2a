"""Sample records on the CPU (csrc/bdpt_math.h bdpt_sample_record, the function
bdpt_sample_records_kernel runs per table position): its host build, with a main of its own
(tests/native/sample_records_check.c), run on the oracle's seed-0 table equals the NumPy float32
restatement (tests/sample_records_ref.py) bit for bit -- on the first and the last 4,096
positions (the last one, j = RAND_N - 6, included), on a seeded sample of 200,000 positions, and
on every position whose five entries include a 0 or a 1, if the table holds any."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import REPO
from sample_records_ref import records

RAND_N = 4096 * 1876
M5 = RAND_N - 5                      # positions j = 0 .. RAND_N - 6


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("srec") / "sample_records_check"
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-Wall", "-o", str(out),
                           os.path.join(REPO, "tests", "native", "sample_records_check.c"), "-lm"])
    return str(out)


@pytest.fixture(scope="module")
def table():
    t = oracle.mt607(0)
    assert t.dtype == np.float32 and t.shape == (RAND_N,)
    return t


def _native(exe, table, pos, tmp_path):
    tp, pp, op = tmp_path / "table.f32", tmp_path / "pos.u32", tmp_path / "out.f32"
    table.tofile(tp)
    np.asarray(pos, np.uint32).tofile(pp)
    r = subprocess.run([exe, str(tp), str(pp), str(op)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    return np.fromfile(op, np.float32).reshape(len(pos), 8)


def test_host_build_equals_restatement(exe, table, tmp_path):
    rng = np.random.default_rng(186)
    edge = np.flatnonzero((table == 0) | (table == 1))
    around = (edge[:, None] - np.arange(5)[None, :]).ravel()          # the entry as u0 .. u4
    around = around[(around >= 0) & (around < M5)]
    pos = np.concatenate([np.arange(4096), np.arange(M5 - 4096, M5), rng.integers(0, M5, 200000), around])
    assert pos.max() == RAND_N - 6 and pos.min() == 0
    got = _native(exe, table, pos, tmp_path)
    want = records(table, pos)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (bad.size, pos[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the records are what they are documented to be: u2 and u0 copied, a unit light sample
    assert np.array_equal(got[:, 3], table[pos + 2]) and np.array_equal(got[:, 7], table[pos])
    assert np.abs((got[:, 4:7].astype(np.float64) ** 2).sum(axis=1) - 1).max() < 1e-6


def test_edge_entries(exe, tmp_path):
    """Entries 1 (the table's largest value, y = 2^32 - 1) and the smallest, 2^-32, in every role:
    sqrt(1 - 1) = 0, zz = -1 with a clamped root, the angle 2 pi."""
    vals = np.float32([1.0, 2.0 ** -32, 0.5, 0.25, 1.0 - 2.0 ** -24, 0.75, 0.0])
    rng = np.random.default_rng(5)
    t = vals[rng.integers(0, len(vals), 4096 + 4)]
    pos = np.arange(4096)
    got = _native(exe, t, pos, tmp_path)
    want = records(t, pos)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
