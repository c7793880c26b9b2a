"""bench.py end to end on one GPU, on a small frame: the JSON line's contract fields, and the
30000-pass counter cap of the path kernel (device.cu:607) -- a run whose steps would cross it
resets the accumulation before the step that would (so every timed step renders all of its
passes) and the frame's counters hold exactly the passes since that reset."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], cwd=REPO,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_crosses_counter_cap():
    # (tuning + 1 warm-up + 240 timed steps) x 128 passes > 30,000: one reset
    d = run_bench("--scene", "simple", "--width", "96", "--height", "64", "--passes", "128",
                  "--steps", "240", "--warmup", "1", "--no-cpu-baseline")
    cfg = d["config"]
    steps = d["tune_steps"] + 1 + 240
    assert 30000 < steps * 128 < 2 * 30000
    assert cfg["accum_resets"] == 1
    assert cfg["spp_total"] == steps * 128 - 30000 // 128 * 128
    assert d["n_gpus"] == 1 and d["steps"] == 240 and d["value"] > 0
    assert cfg["samples_per_step"] == 97 * 65 * 128
    for k in ("metric", "unit", "ms_per_step", "higher_is_better", "scaling", "dtype", "roofline", "cpu_baseline"):
        assert k in d


def test_dump_outputs_is_the_last_steps_frame(tmp_path):
    """--dump-outputs writes the frame the timed path holds after its last timed step: float32
    files that equal, bit for bit, the oracle's frame for every pass the run rendered (tuning,
    warm-up and timed steps), and that a second run of the same workload writes again.  The plain
    run carries no CPU baseline; the second run adds --full, which brings it back and changes
    nothing about the frame."""
    import numpy as np

    import gpu_bidirectional_raytracer_amd as g
    import oracle

    args = ("--scene", "simple", "--width", "32", "--height", "24", "--passes", "4", "--steps", "2", "--warmup", "1")
    a, b = tmp_path / "a", tmp_path / "b"
    d = run_bench(*args, "--dump-outputs", str(a))
    full = run_bench(*args, "--dump-outputs", str(b), "--full", "--cpu-seconds", "0.2", "--no-smt-probe")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None and "speedup_vs_cpu" not in d
    assert full["cpu_baseline"]["value"] > 0 and full["speedup_vs_cpu"] > 0

    W, H = 33, 25
    npass = (d["tune_steps"] + 1 + 2) * 4
    assert d["config"]["spp_total"] == npass
    cam, sp = g.read_scene(os.path.join(REPO, "assets", "scenes", "simple.scn"))
    g.update_camera(cam, W, H)
    sched = g.PassScheduler()
    sched.light()
    sid, vlp = sched.next(npass)
    rnd = oracle.mt607(0)
    ocol, ocnt, opx = oracle.path_passes(sp, rnd, cam, W, H, oracle.light_pass(sp, rnd, 0), sid, vlp)
    want = {"colors": ocol.reshape(-1, 3), "counter": ocnt.reshape(-1), "pixels": opx.reshape(-1, 4)[:, :3]}
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["colors.npy", "counter.npy", "pixels.npy"]
    for name, ref in want.items():
        got = np.load(a / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got, ref.astype(np.float32)), name
        assert np.array_equal(got, np.load(b / (name + ".npy"))), name
    assert (want["counter"] == npass).all() and want["colors"].any()
