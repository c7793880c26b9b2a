"""The queued-call scenarios of tests/queued_calls.py on the CPU backend, against the full-frame oracle.

Nothing is queued here: the CPU backend finishes every call before it returns.  What this module
holds to the oracle is the harness itself -- every step, every `expect` chain (masks, shard rows,
scene, camera and light edits, the mark, the estimate, the checkpoint) and every product's numpy
statement -- so that a difference seen on the GPU is a finding about the GPU's call ordering and not
about the test.  The frame is 33 x 25 (2 x 4 tiles, the last column 1 pixel wide, the last row 1
high), calls of 12 and 8 passes."""
import ctypes

import numpy as np
import pytest

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g
import queued_calls as qc
from reproject_common import hist_dict

W, H, N1, N2 = 33, 25, 12, 8


def _run(steps, tmp_path, scene="cornell"):
    return qc.run(scene, steps, qc.CPU, True, tmpdir=str(tmp_path), width=W, height=H)


def test_calls_in_flight_abi():
    """0 on the CPU backend, BDPT_EINVAL for NULL."""
    lib, n = g._lib.lib, ctypes.c_int(7)
    assert lib.bdpt_calls_in_flight(None, ctypes.byref(n)) == g._lib.BDPT_EINVAL
    cam, sp = g.read_scene(qc.os.path.join(qc.SCENES, "cornell.scn"))
    g.update_camera(cam, W, H)
    s = g.PassScheduler()
    s.light()
    with g.Renderer(sp, W, H, cam, device=qc.CPU) as r:
        assert lib.bdpt_calls_in_flight(r._h, None) == g._lib.BDPT_EINVAL
        assert r.calls_in_flight() == 0
        r.light_pass(0)
        r.path_passes(*s.next(3), sync=False)
        assert r.calls_in_flight() == 0


@pytest.mark.parametrize("a", qc.M, ids=qc.label)
def test_pairs(a, tmp_path):
    steps = qc.pairs(a, N1, N2)
    got = _run(steps, tmp_path)
    qc.same_reads(got["reads"], qc.expect("cornell", steps, None, W, H)[0], f"cpu, {qc.label(a)} then every mode")


def test_pairs_bvh_scene(tmp_path):
    steps = qc.pairs(qc.M_BVH[2], N1, N2, qc.M_BVH)
    got = _run(steps, tmp_path, "synthetic64")
    qc.same_reads(got["reads"], qc.expect("synthetic64", steps, None, W, H)[0], "cpu, synthetic64")


def test_more_calls_than_ring_slots(tmp_path):
    steps = qc.ring(8)
    got = _run(steps, tmp_path)
    want, _ = qc.expect("cornell", steps, None, W, H)
    qc.same_reads(got["reads"], want, "cpu, ring")
    _, cnt0 = am.uneven_state(W, H, 7)
    am.same(got["reads"][0]["counter"], am.closed_form_counter(cnt0, qc.passes_per_pixel(steps, W, H)),
            "cpu, ring: counter vs the closed form")


@pytest.mark.parametrize("k,op", qc.CASES, ids=[f"{qc.label(qc.A_SET[k])}-{qc.op_label(op)}" for k, op in qc.CASES])
def test_op_between_calls(k, op, tmp_path):
    a = qc.A_SET[k]
    b = (("fused_paired", "one_per_lane")[(k + qc.OPS.index(op)) % 2], None)
    steps = qc.behind(a, op, b, N1, N2)
    got = _run(steps, tmp_path)
    want, frames = qc.expect("cornell", steps, None, W, H)
    what = f"cpu, {qc.label(a)}, {qc.op_label(op)}, {qc.label(b)}"
    qc.same_reads(got["reads"], want, what)
    last, seen = got["reads"][-1], frames[-2]                  # the frame the op saw: after A's call
    if op[0] == "mark":
        qc.same_bytes(last["mark"][0], seen[0], f"{what}: the mark's colours vs the frame after A")
        qc.same_bytes(last["mark"][1], seen[1], f"{what}: the mark's counts vs the frame after A")
    if op[0] == "capture":
        qc.same_bytes(last["history"][0], seen[0], f"{what}: the captured colours vs the frame after A")
        qc.same_bytes(last["history"][1], seen[1].astype(np.float32), f"{what}: the captured weight")
    if op[0] == "service":
        pre = got["reads"][0]
        inp = qc.Inputs("cornell", W, H, 0)
        hist = hist_dict(inp.cam, pre["history"][0], pre["history"][1], last["guides"])
        qc.check_service(op[1], last, seen, pre["mark"], hist, inp.sp)


def test_masked_call_on_a_shard_is_refused(tmp_path):
    steps = (("shard", 0, 2, 16), ("passes", N2, "one_per_lane", "A"))
    with pytest.raises(g.BdptError) as e:
        _run(steps, tmp_path)
    assert e.value.code == g._lib.BDPT_EINVAL
