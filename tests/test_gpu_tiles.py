"""Path passes over a tile mask (include/bdpt.h bdpt_path_passes_tiles) on the GPU, in every kernel
mode that takes a tile list -- fused with paired and unpaired loads, two, four and one pass(es) per
lane, a fixed S, the precompiled builds and the BVH build (tests/accum_modes.py) -- on a 97 x 65
frame (4 x 9 tiles, the last column one pixel wide, the last row one pixel high) that starts from an
uneven accumulation state.  A masked call must leave the oracle's unmasked result from the same
state where the mask says and the state before the call elsewhere, bit for bit
(tests/tiles_common.py), and every case proves what ran: the tile list, no pools and no units, the
stream count, the build and the launch count.  Then forced pools and units (ignored under a mask),
the auto stream mode's measurement (untouched by masked calls), the empty and the full mask, and
the adaptive RenderUntil against the CPU backend."""
import pytest

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g
import tiles_common as tc

pytestmark = pytest.mark.gpu

MODES = ["fused_paired", "fused_unpaired", "two_per_lane", "four_per_lane", "one_per_lane", "fixed_s3",
         "precompiled_fused", "precompiled_one_per_lane", "bvh_fused", "bvh_one_per_lane"]


def _scene(mode):
    return "synthetic64" if mode.bvh else "cornell"


@pytest.mark.parametrize("name", MODES)
def test_masked_calls_every_mode(gpu, name, monkeypatch):
    mode = am.BY_NAME[name]
    tc.check_masked(mode, _scene(mode), (("A", 9), ("B", 11)), gpu, monkeypatch)


@pytest.mark.parametrize("name", ["two_per_lane", "fused_paired"])
def test_masked_call_cut_into_launches(gpu, name, monkeypatch):
    """20 passes under BDPT_MAX_LAUNCH_PASSES=6: four launches of 5 over one tile list; the third
    reuses a half of the radiance buffer (masked_call asserts the count from launch_passes)."""
    mode = am.BY_NAME[name]
    assert am.launch_passes(20, 6, mode.last_streams(20) == 1) == (5, 4)
    tc.check_masked(mode, "cornell", (("A", 20),), gpu, monkeypatch, limit=6)


@pytest.mark.parametrize("name", ["pool2", "units3"])
def test_forced_pools_and_units_are_ignored_under_a_mask(gpu, name, monkeypatch):
    mode = am.BY_NAME[name]
    am.force_env(mode, None, monkeypatch)
    sc = am.Scenario("tiles", "cornell", ())
    cam, sp = am.load_scene(sc)
    steps = (("A", 9), ("F", 9))           # the second call is unmasked: every pixel
    sid, vlp = am.schedule(9 + 9)
    with g.Renderer(sp, tc.W, tc.H, cam, device=gpu) as r:
        r.light_pass(0)
        r.write_radiance(*am.uneven_state(tc.W, tc.H, 7))
        state0 = tc.read_state(r)
        r.set_streams(9)
        r.path_passes(sid[:9], vlp[:9], tiles=tc.mask("A"))
        assert "tile_list" in r.last_features, r.last_features
        assert "pixel_pools" not in r.last_features and "unit_fold" not in r.last_features, r.last_features
        assert r.last_streams == 9 and r.last_specialized
        tc.same_state(tc.read_state(r), tc.chain("cornell", state0, steps)[0], f"{name} forced, mask A")
        # the unmasked call right after runs the forced mode, from the masked call's state
        r.path_passes(sid[9:], vlp[9:])
        assert mode.feature in r.last_features and "tile_list" not in r.last_features, r.last_features
        tc.same_state(tc.read_state(r), tc.chain("cornell", state0, steps)[1], f"{name} forced, unmasked call after")


def test_masked_calls_leave_the_measurement_alone(gpu, monkeypatch):
    """Auto mode, still measuring: the roles the unmasked calls run (seen as last_streams and
    features) and stream_choice are the same with masked calls interleaved as without."""
    for var in ("BDPT_POOL", "BDPT_UNITS", "BDPT_MAX_LAUNCH_PASSES", "BDPT_STREAMS_TUNE"):
        monkeypatch.delenv(var, raising=False)
    sc = am.Scenario("tiles", "cornell", ())
    cam, sp = am.load_scene(sc)
    sid, vlp = am.schedule(8)

    def roles(interleave):
        seen = []
        with g.Renderer(sp, tc.W, tc.H, cam, device=gpu) as r:
            r.light_pass(0)
            for k in range(11):
                if interleave:
                    r.path_passes(sid, vlp, tiles=tc.mask("A" if k % 2 else "B"))
                    assert "tile_list" in r.last_features
                    assert r.last_streams == (4 if k < 10 or not r.stream_choice & am.FUSED else 1)
                    seen.append(("masked", r.stream_choice & am.DECIDED))
                r.path_passes(sid, vlp)
                f = [x for x in r.last_features if x != "tile_list"]
                assert "tile_list" not in r.last_features
                # while measuring (the first ten calls) there is no choice; the eleventh decides
                seen.append((r.last_streams if k < 10 else None, tuple(f) if k < 10 else None,
                             r.stream_choice if k < 10 else r.stream_choice & am.DECIDED))
        return seen

    plain, mixed = roles(False), roles(True)
    assert [s for s in mixed if s[0] != "masked"] == plain
    assert [s[0] for s in plain[:10]] == [4, 1, 2, 4, 1, 2, 8, 8, 4, 4]
    assert all(s[2] == 0 for s in plain[:10]) and plain[10][2] == am.DECIDED
    assert all(s[1] == 0 for s in mixed if s[0] == "masked")          # no decision at any masked call's end


def test_empty_and_full_masks(gpu, monkeypatch):
    am.force_env(am.BY_NAME["one_per_lane"], None, monkeypatch)
    sc = am.Scenario("tiles", "cornell", ())
    cam, sp = am.load_scene(sc)
    sid, vlp = am.schedule(9)
    with g.Renderer(sp, tc.W, tc.H, cam, device=gpu) as r:
        r.light_pass(0)
        r.set_streams(-1)
        r.write_radiance(*am.uneven_state(tc.W, tc.H, 7))
        state0 = tc.read_state(r)
        r.kernel_timing(reset=True)
        r.path_passes(sid, vlp, tiles=tc.mask("Z"))
        assert r.kernel_timing()[1] == 0
        tc.same_state(tc.read_state(r), state0, "all-zero mask")
        r.path_passes(sid, vlp, tiles=tc.mask("F"))
        assert "tile_list" in r.last_features
        tc.same_state(tc.read_state(r), tc.chain("cornell", state0, (("F", 9),))[0], "all-one mask")
        with pytest.raises(g.BdptError):
            r.set_shard(1, 3, 8)
            r.path_passes(sid, vlp, tiles=tc.mask("A"))


def test_adaptive_render_until_matches_the_cpu(gpu):
    est, col, cnt, px = tc.adaptive_run(gpu, "cornell", 0.05)
    cest, ccol, ccnt, cpx = tc.adaptive_run(-1, "cornell", 0.05)
    print(f"GPU: passes {est['passes']}, pixel_passes {est['pixel_passes']}")
    assert est["converged"] and est["passes"] == 384 and est["pixel_passes"] == 480864
    assert est["retired_at"].tolist() == [[96, 128, 64], [128, 192, 48], [96, 192, 96], [96, 104, 96], [104, 192, 120],
                                          [128, 384, 24], [96, 96, 96]]
    am.same(est["retired_at"], cest["retired_at"], "retired_at")
    am.same(est["retired_error"], cest["retired_error"], "retired_error")
    tc.same_state((col, cnt, px), (ccol, ccnt, cpx), "GPU frame against the CPU backend's")
