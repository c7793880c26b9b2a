"""Call sequences issued without waiting for the device (path_passes(sync=False), as bench.py and an
interactive host issue them) against the oracle: the host layer's ordering between queued calls --
the two radiance halves and their events, the fold stream beside the next path kernel, the pool
streams, the ring of call slots with a masked call's tile list, and join_fold in front of everything
that reads or rewrites the frame.  The scenarios and the harness are tests/queued_calls.py; the same
scenarios run on the CPU backend in tests/test_queued_calls_cpu.py, which holds the harness itself
to the oracle.

Every case proves, from getters that do not synchronise, which kernels ran, and from
Renderer.calls_in_flight() that the device was still busy with the earlier call when the next one
was issued: a case whose queue had drained fails, it does not pass untested.  The frame is 161 x 97
(6 x 13 tiles, the last column 1 pixel wide and the last row 1 high); every comparison is on bits."""
import numpy as np
import pytest

import accum_modes as am
import queued_calls as qc
from reproject_common import hist_dict

pytestmark = pytest.mark.gpu
W, H = qc.W, qc.H


def _busy(in_flight, what, only=None):
    """Every recorded probe (or the one of step `only`) saw at least one call in flight."""
    seen = [x for x in in_flight if only is None or x[0] == only]
    assert seen, f"{what}: no probe recorded"
    print(f"{what}: calls in flight {[(k, n) for k, _, n in seen]}")
    assert not qc.drained(seen), f"{what}: {qc.drained(seen)}"


def _probes(in_flight):
    return [x for x in in_flight if x[1][0] == "probe"]


def _launches(got, steps, what):
    want = sum(qc.passes_launches(s) for s in steps if s[0] == "passes")
    assert got["launches"] == (want, want), f"{what}: launches (planned, counted) {got['launches']}, the calls' sum {want}"


# ---- a. every ordered pair of modes ---------------------------------------------------------------

@pytest.mark.parametrize("a", qc.M, ids=qc.label)
def test_every_mode_behind_this_one(gpu, a, monkeypatch, tmp_path):
    """For every B: A's long call, B's call queued behind it, the whole frame against the oracle.
    The probe between the two calls must find A's call running; the one after B's call is printed
    (2: A's was still running when B's had been issued -- so for every A but the masked one_per_lane,
    whose 1024 passes on half the tiles are nearly over by then)."""
    steps = qc.pairs(a, qc.n1_of(a), qc.N2)
    what = f"{qc.label(a)} ({qc.n1_of(a)} passes) then every mode ({qc.N2})"
    got = qc.run("cornell", steps, gpu, True, monkeypatch, str(tmp_path))
    _busy(_probes(got["in_flight"]), what)
    _launches(got, steps, what)
    want, _ = qc.expect("cornell", steps)
    assert len(got["reads"]) == len(qc.M)
    for k, b in enumerate(qc.M):                              # read by read: a failure names its pair
        qc.same_frame(got["reads"][k], want[k], f"{qc.label(a)} then {qc.label(b)}")


@pytest.mark.parametrize("a", qc.M_BVH, ids=qc.label)
def test_every_bvh_mode_behind_this_one(gpu, a, monkeypatch, tmp_path):
    steps = qc.pairs(a, qc.n1_of(a), qc.N2, qc.M_BVH)
    what = f"synthetic64: {qc.label(a)} ({qc.n1_of(a)} passes) then every BVH mode"
    got = qc.run("synthetic64", steps, gpu, True, monkeypatch, str(tmp_path))
    _busy(_probes(got["in_flight"]), what)
    _launches(got, steps, what)
    want, _ = qc.expect("synthetic64", steps)
    for k, b in enumerate(qc.M_BVH):
        qc.same_frame(got["reads"][k], want[k], f"synthetic64: {qc.label(a)} then {qc.label(b)}")


# ---- b. more calls than ring slots ----------------------------------------------------------------

def test_more_queued_calls_than_ring_slots(gpu, monkeypatch, tmp_path):
    """Eleven calls and one read: every slot of the ring is reused (a masked call's tile list with
    another length), a radiance half is reused inside a queued call, and the counters that start
    just below the cap reach it in different queued launches."""
    steps = qc.ring(qc.N_RING)
    got = qc.run("cornell", steps, gpu, True, monkeypatch, str(tmp_path))
    probes = _probes(got["in_flight"])
    _busy(probes[1:], "ring")                                 # (the first call is the short one)
    assert max(n for _, _, n in probes) >= 2, f"ring: never two calls in flight: {[n for _, _, n in probes]}"
    _launches(got, steps, "ring")
    want, _ = qc.expect("cornell", steps)
    qc.same_frame(got["reads"][0], want[0], "ring")
    _, cnt0 = am.uneven_state(W, H, 7)
    am.same(got["reads"][0]["counter"], am.closed_form_counter(cnt0, qc.passes_per_pixel(steps, W, H)),
            "ring: counter vs the closed form")


# ---- c. every state-changing or frame-reading call behind running passes --------------------------

def _behind(gpu, monkeypatch, tmp_path, scene, a, op, b, n1):
    steps = qc.behind(a, op, b, n1, qc.N2)
    at = len(steps) - 3                                       # the op under test, not a prefix's
    what = f"{scene}: {qc.label(a)} ({n1}), {qc.op_label(op)}, {qc.label(b)}"
    (tmp_path / "q").mkdir()
    (tmp_path / "t").mkdir()
    got = qc.run(scene, steps, gpu, True, monkeypatch, str(tmp_path / "q"))
    twin = qc.run(scene, steps, gpu, False, monkeypatch, str(tmp_path / "t"))
    _busy(got["in_flight"], what, only=at)
    _launches(got, steps, what)
    qc.same_reads(got["reads"], twin["reads"], f"{what}: queued vs synchronised")
    want, _ = qc.expect(scene, steps, qc.ROWS)
    for k in range(len(want)):
        qc.same_frame(twin["reads"][k], want[k], f"{what}: the synchronised twin vs the oracle, read {k + 1}", qc.ROWS)
        qc.same_frame(got["reads"][k], want[k], f"{what}: queued vs the oracle, read {k + 1}", qc.ROWS)
    return steps, got, twin, what


@pytest.mark.parametrize("k,op", qc.CASES, ids=[f"{qc.label(qc.A_SET[k])}-{qc.op_label(op)}" for k, op in qc.CASES])
def test_call_behind_running_passes(gpu, k, op, monkeypatch, tmp_path):
    a = qc.A_SET[k]
    b = (("fused_paired", "one_per_lane")[(k + qc.OPS.index(op)) % 2], None)
    steps, got, twin, what = _behind(gpu, monkeypatch, tmp_path, "cornell", a, op, b, qc.n1_of(a))
    last, seen = got["reads"][-1], twin["frames"][-2]         # what the op saw: the twin's frame after A
    if op[0] == "mark":
        qc.same_bytes(last["mark"][0], seen[0], f"{what}: the mark's colours vs the frame after A")
        qc.same_bytes(last["mark"][1], seen[1], f"{what}: the mark's counts vs the frame after A")
    if op[0] == "estimate":
        mc, mn = got["reads"][0]["mark"]
        qc.same_estimate(last["estimate"], qc.np_noise(seen[0], seen[1], mc, mn, remark=True), f"{what}: vs numpy")
    if op[0] == "capture":
        qc.same_bytes(last["history"][0], seen[0], f"{what}: the captured colours vs the frame after A")
        qc.same_bytes(last["history"][1], seen[1].astype(np.float32), f"{what}: the captured weight")
    if op[0] == "service":
        pre = got["reads"][0]
        inp = qc.Inputs("cornell", W, H, 0)
        hist = hist_dict(inp.cam, pre["history"][0], pre["history"][1], last["guides"])
        qc.check_service(op[1], last, seen, pre["mark"], hist, inp.sp)


@pytest.mark.parametrize("a,op,b", [("bvh_one_per_lane", ("traversal", "brute"), "precompiled_one_per_lane"),
                                    ("precompiled_one_per_lane", ("traversal", "bvh"), "bvh_fused")],
                         ids=["bvh-to-brute", "brute-to-bvh"])
def test_traversal_change_behind_running_passes(gpu, a, op, b, monkeypatch, tmp_path):
    _behind(gpu, monkeypatch, tmp_path, "synthetic64", (a, None), op, (b, None), qc.N1_BVH)


def test_masked_call_on_a_shard_is_refused(gpu, monkeypatch, tmp_path):
    import gpu_bidirectional_raytracer_amd as g
    steps = (("passes", qc.N2, "two_per_lane", None), ("shard", 0, 2, 16), ("passes", qc.N2, "one_per_lane", "A"))
    with pytest.raises(g.BdptError) as e:
        qc.run("cornell", steps, gpu, True, monkeypatch, str(tmp_path))
    assert e.value.code == g._lib.BDPT_EINVAL


# ---- d. a group -----------------------------------------------------------------------------------

def test_group_of_three_queued(gpu, monkeypatch, tmp_path):
    """Six queued calls over three modes on devices=[gpu] * 3 with a reset and a scene edit in the
    middle, against the one-device oracle chain."""
    n = qc.N_GROUP                                            # (the fused calls are the long ones: the ops follow them)
    steps = (("passes", n, "two_per_lane", None), ("passes", n, "fused_paired", None), ("probe",), ("reset",),
             ("passes", n, "one_per_lane", None), ("passes", n, "fused_paired", None), ("probe",), ("scene", 6, -5.0),
             ("passes", n, "two_per_lane", None), ("passes", n, "one_per_lane", None), ("read",))
    got = qc.run("cornell", steps, gpu, True, monkeypatch, str(tmp_path), devices=[gpu] * 3)
    _busy([x for x in got["in_flight"] if x[1][0] in ("probe", "reset", "scene")], "group of three")
    want, _ = qc.expect("cornell", steps)
    qc.same_frame(got["reads"][0], want[0], "group of three")


# ---- e. closing with work queued ------------------------------------------------------------------

def test_close_with_calls_queued(gpu, monkeypatch, tmp_path):
    """bdpt_destroy waits for the fold stream, the pool streams and the context's stream before it
    frees anything; a context made right afterwards on the same device renders as ever."""
    steps = (("passes", qc.n1_of(("pool_overlap", None)), "pool_overlap", None),
             ("passes", qc.n1_of(("two_per_lane", None)), "two_per_lane", None), ("probe",))
    got = qc.run("cornell", steps, gpu, True, monkeypatch, str(tmp_path))
    _busy(got["in_flight"], "before the close")
    after = (("passes", 8, "fused_paired", None), ("read",))
    got = qc.run("cornell", after, gpu, True, monkeypatch, str(tmp_path))
    qc.same_frame(got["reads"][0], qc.expect("cornell", after)[0][0], "a new context after the close")
