"""The path kernels across sphere counts and emitter positions (tests/count_scenes.py; the scenes
and what they reach are proven on the CPU by tests/test_count_scenes_cpu.py).

The scene-specialised builds fold the sphere count N and the 64-bit emitter mask into their code:
the straight-line part-full shadow rounds exist per (lane-group count, list) where pf_fits holds,
mask a partial last iteration, shift the mask as 32 bits up to N = 32 and as 64 above, skip the
emitter test in iterations without an emitter and run a second list of the non-emitters where
vac_list says so.  count_scenes.CASES holds one scene for every such class and the counts 1, 2,
16, 17, 32, 33, 63 and 64, with emitters at index 0, 31, 32, 63 and N - 1 whose shadow on the
frame the CPU module has counted.

  * Specialised kernels: every case in the fused kernel, a fixed S = 3 pass stream and the ordered
    in-kernel fold (and pixel pools for the counts above 32 and one small one), 16 passes in one
    call, on the tiny frames of 1, 2, 4, 8, 16 and 32 pixels -- rounds of at most 2, 4, ..., 64
    rays: every lane-group count --, on three more of 2, 3 and 4 pixels and on 45 x 31, with full waves, a part-full second round of
    VLP rays alone and both packed edges.
  * Masked launches (the BDPT_TILES builds) of two cases above 32 spheres.
  * The precompiled kernels bdpt_path_kernel_t<1..16, *> and the generic one at 17 spheres, each
    with the emitter at index N - 1, fused and one pass per lane.
  * The light pass at current_sample 0 and 3 and the first-hit buffers of every case.
  * The tree traversal of the cases that have a tree (emitter flags up to index 63).

Every comparison is on the bits of colours, counters and pixels against the oracle, computed once
per (case, frame); there is no tolerance.  The geometry does not depend on the frame, so a (case,
mode) compiles once and the other frames load the cached build."""
import numpy as np
import pytest

import accum_modes as am
import count_scenes as cs
import gpu_bidirectional_raytracer_amd as g
import tiles_common as tc

pytestmark = pytest.mark.gpu

MODES = ["fused_paired", "fixed_s3", "units3"]
POOL_CASES = [c for c in cs.CASES if c[0] > 32] + [(7, (6,))]
FRAMES = cs.TINY_FRAMES + cs.MORE_TINY + [cs.FULL_FRAME]
W, H = cs.FULL_FRAME
MASKED = [((49, (48,)), "fixed_s3"), ((64, (8, 32, 33, 63)), "fused_paired")]
TREE_CASES = [c for c in cs.CASES if c[0] >= 32]            # 26 or more small spheres: bdpt_build_bvh makes a tree


def _check(got, want, what):
    print(f"{what}: {int((am.bits(got[0]) != am.bits(want[0])).sum())} colour values, "
          f"{int((got[1] != want[1]).sum())} counters, {int((got[2] != want[2]).any(-1).sum())} pixels differ")
    for a, b, part in zip(got, want, ("colors", "counter", "pixels")):
        am.same(a, b, f"{what}: {part}")


def _specialised(case, name, gpu, monkeypatch):
    mode = am.BY_NAME[name]
    am.force_env(mode, None, monkeypatch)
    monkeypatch.delenv("BDPT_JIT_FLAGS", raising=False)
    sid, vlp = cs.schedule(cs.NPASS)
    for w, h in FRAMES:
        cam, sp = cs.load(case, w, h)
        what = f"{cs.case_id(case)} {name} {w}x{h}"
        with g.Renderer(sp, w, h, cam, device=gpu) as r:
            r.set_specialize(True)
            r.set_traversal("brute")
            r.light_pass(0)
            am._call(r, mode, sid, vlp, None)          # asserts the mode, the launch count, specialised
            assert "specialized" in r.last_features, f"{what}: {r.last_features}: {r.specialize_status!r}"
            got = tc.read_state(r)
        _check(got, cs.expected(case, w, h, cs.NPASS), what)


@pytest.mark.parametrize("name", MODES)
@pytest.mark.parametrize("case", cs.CASES, ids=cs.case_id)
def test_specialised_kernels(gpu, case, name, monkeypatch):
    _specialised(case, name, gpu, monkeypatch)


@pytest.mark.parametrize("case", POOL_CASES, ids=cs.case_id)
def test_specialised_pixel_pools(gpu, case, monkeypatch):
    _specialised(case, "pool2", gpu, monkeypatch)


@pytest.mark.parametrize("case,name", MASKED, ids=lambda v: cs.case_id(v) if isinstance(v, tuple) else v)
def test_masked_launches(gpu, case, name, monkeypatch):
    """One call over a checkerboard of the 2 x 4 tiles: the oracle's frame where the mask says,
    the state before the call elsewhere."""
    mode = am.BY_NAME[name]
    am.force_env(mode, None, monkeypatch)
    cam, sp = cs.load(case, W, H)
    sid, vlp = cs.schedule(cs.NPASS)
    tiles = tc.mask("A", -(-W // tc.TW), -(-H // tc.TH))
    assert 0 < tiles.sum() < tiles.size
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.set_specialize(True)
        r.set_traversal("brute")
        r.light_pass(0)
        before = tc.read_state(r)
        tc.masked_call(r, mode, sid, vlp, None, tiles)
        assert "specialized" in r.last_features, f"{r.last_features}: {r.specialize_status!r}"
        got = tc.read_state(r)
    m = tc.pixel_mask(tiles, W, H)
    full = cs.expected(case, W, H, cs.NPASS)
    want = (np.where(m[..., None], full[0], before[0]), np.where(m, full[1], before[1]),
            np.where(m[..., None], full[2], before[2]))
    _check(got, want, f"{cs.case_id(case)} {name} masked")


@pytest.mark.parametrize("streams", [1, -1])
@pytest.mark.parametrize("case", cs.PRECOMPILED, ids=cs.case_id)
def test_precompiled_kernels(gpu, case, streams):
    cam, sp = cs.load(case, W, H)
    sid, vlp = cs.schedule(cs.SHORT)
    what = f"{cs.case_id(case)} precompiled streams={streams}"
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.set_specialize(False)
        r.set_traversal("brute")
        r.set_streams(streams)
        r.light_pass(0)
        r.path_passes(sid, vlp)
        assert not r.last_specialized, f"{what}: {r.specialize_status!r}"
        assert r.last_traversal == "brute" and "specialized" not in r.last_features, f"{what}: {r.last_features}"
        assert r.last_streams == (1 if streams == 1 else len(sid)), f"{what}: {r.last_streams}"
        got = tc.read_state(r)
    _check(got, cs.expected(case, W, H, cs.SHORT), what)


@pytest.mark.parametrize("case", cs.CASES, ids=cs.case_id)
def test_light_pass_and_first_hit(gpu, case):
    cam, sp = cs.load(case, W, H)
    sid, _ = cs.schedule(cs.NPASS)
    what = cs.case_id(case)
    with g.Renderer(sp, W, H, cam, device=gpu) as r, g.Renderer(sp, W, H, cam, device=-1) as cpu:
        for sample, after in ((0, None), (3, 0)):          # entries no light ray writes keep light_pass(0)'s
            r.light_pass(sample)
            am.same(r.read_lightpaths().view(np.float32), cs.light_points(case, sample, after).view(np.float32),
                    f"{what}: light points of light_pass({sample})")
        cpu.generate_rand(15)                              # the table light_pass(3) left
        for s in (None, int(sid[0]), int(sid[7])):
            got, want = r.render_aov(sid=s), cpu.render_aov(sid=s)
            for k in g.AOV_PLANES:
                am.same(got[k], want[k], f"{what}: render_aov(sid={s}) {k}")


@pytest.mark.parametrize("name", ["bvh_fused", "bvh_one_per_lane"])
@pytest.mark.parametrize("case", TREE_CASES, ids=cs.case_id)
def test_tree_traversal(gpu, case, name, monkeypatch):
    mode = am.BY_NAME[name]
    am.force_env(mode, None, monkeypatch)
    cam, sp = cs.load(case, W, H)
    sid, vlp = cs.schedule(cs.NPASS)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        assert r.has_bvh
        r.set_specialize(False)
        r.set_traversal("bvh")
        r.light_pass(0)
        am._call(r, mode, sid, vlp, None)                  # asserts last_traversal == "bvh"
        got = tc.read_state(r)
    _check(got, cs.expected(case, W, H, cs.NPASS), f"{cs.case_id(case)} {name}")
