"""Path passes over a tile mask (include/bdpt.h bdpt_path_passes_tiles), the per-tile pending counts
(bdpt_noise_tile_pending) and the adaptive RenderUntil built on them, on the CPU backend.  A masked
call must leave, bit for bit, the oracle's unmasked result from the same state where the mask says
and the state before the call elsewhere (tests/tiles_common.py); the adaptive loop must give the
figures derived from an unmasked render and the numpy statement of the estimate."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g
import noise_common as nc
import tiles_common as tc
from conftest import REPO

CPU = -1
# SmallPT(64, 48, cornell).RenderUntil(adaptive=True) with the defaults (threshold 0.05, batch 8)
CORNELL_RETIRED_AT = [[96, 128, 64], [128, 192, 48], [96, 192, 96], [96, 104, 96], [104, 192, 120], [128, 384, 24],
                      [96, 96, 96]]


def _renderer(width=tc.W, height=tc.H, light=True):
    sc = am.Scenario("tiles", "cornell", (), width=width, height=height)
    cam, sp = am.load_scene(sc)
    r = g.Renderer(sp, width, height, cam, device=CPU)
    if light:
        r.light_pass(0)
    return r


@pytest.mark.parametrize("steps", [(("A", 9), ("B", 11)), (("B", 9), ("C", 11)), (("C", 9), ("A", 11))],
                         ids=["A_then_B", "B_then_C", "C_then_A"])
def test_masked_calls_match_the_oracle(steps):
    tc.check_masked(None, "cornell", steps, CPU)


def test_empty_full_and_null_masks():
    sid, vlp = am.schedule(9)
    with _renderer() as r, _renderer() as plain:
        for q in (r, plain):
            q.write_radiance(*am.uneven_state(tc.W, tc.H, 7))
        before = tc.read_state(r)
        r.kernel_timing(reset=True)
        r.path_passes(sid, vlp, tiles=tc.mask("Z"))
        assert r.kernel_timing()[1] == 0, "an all-zero mask must not count as a launch"
        tc.same_state(tc.read_state(r), before, "all-zero mask")
        plain.path_passes(sid, vlp)
        want = tc.read_state(plain)
        r.path_passes(sid, vlp, tiles=tc.mask("F"))
        tc.same_state(tc.read_state(r), want, "all-one mask against an unmasked call")
        assert "tile_list" in r.last_features and "tile_list" not in plain.last_features
        # NULL is bdpt_path_passes
        for q in (r, plain):
            q.write_radiance(*am.uneven_state(tc.W, tc.H, 7))
        rc = g._lib.lib.bdpt_path_passes_tiles(r._h, sid.ctypes.data_as(ctypes.c_void_p), vlp.ctypes.data_as(ctypes.c_void_p),
                                               len(sid), None)
        assert rc == g.BDPT_OK
        tc.same_state(tc.read_state(r), want, "NULL mask against path_passes")
        assert "tile_list" not in r.last_features


def test_error_codes():
    lib, EINVAL, ESTATE = g._lib.lib, g._lib.BDPT_EINVAL, g._lib.BDPT_ESTATE
    sid, vlp = am.schedule(3)
    ps, pv = sid.ctypes.data_as(ctypes.c_void_p), vlp.ctypes.data_as(ctypes.c_void_p)
    m = tc.mask("A")
    pm = m.ctypes.data_as(ctypes.c_void_p)
    with _renderer(light=False) as r:
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, 3, pm) == ESTATE          # no random table yet
        z = tc.mask("Z")
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, 3, z.ctypes.data_as(ctypes.c_void_p)) == ESTATE   # checks first
        r.light_pass(0)
        assert lib.bdpt_path_passes_tiles(r._h, None, pv, 3, pm) == EINVAL
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, -1, pm) == EINVAL
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, 0, pm) == g.BDPT_OK
        r.set_shard(1, 3, 8)
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, 3, pm) == EINVAL          # sharded
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, 3, None) == g.BDPT_OK     # NULL: a plain sharded call
        r.set_shard(0, 1, 8)
        assert lib.bdpt_path_passes_tiles(r._h, ps, pv, 3, pm) == g.BDPT_OK
        with pytest.raises(ValueError):
            r.path_passes(sid, vlp, tiles=np.ones((3, 3), bool))


def test_tile_pending_is_the_estimates():
    Wn, Hn = 65, 49
    col, cnt, mc, mn = nc.case(Wn, Hn)
    with _renderer(Wn, Hn) as r:
        tp = np.empty((7, 3), np.uint32)
        assert g._lib.lib.bdpt_noise_tile_pending(r._h, tp.ctypes.data_as(ctypes.c_void_p)) == g._lib.BDPT_ESTATE
        with pytest.raises(g.BdptError):
            r.noise_tile_pending()
        r.write_radiance(col, cnt)
        r.noise_write_mark(mc, mn)
        est = r.noise_estimate()
        assert g._lib.lib.bdpt_noise_tile_pending(r._h, None) == g._lib.BDPT_EINVAL
        want = nc.np_noise(col, cnt, mc, mn)
        am.same(r.noise_tile_pending(), want["tile_pending"], "tile_pending")
        assert int(r.noise_tile_pending().sum()) == est["pending_pixels"] > 0


def _check_adaptive(scene, threshold, passes, pixel_passes, retired_at=None, min_passes=0):
    est, col, cnt, px = tc.adaptive_run(CPU, scene, threshold, min_passes)
    d_at, d_err, d_pp, d_passes, d_col, d_cnt, d_px = tc.adaptive_derived(scene, threshold, min_passes)
    print(f"{scene} {threshold}: passes {est['passes']}, pixel_passes {est['pixel_passes']}, derived {d_passes}, {d_pp}")
    assert est["converged"] and est["passes"] == d_passes and est["pixel_passes"] == d_pp
    assert est["retired_at"].dtype == np.int32 and est["retired_error"].dtype == np.float32
    am.same(est["retired_at"], d_at, "retired_at against the derivation")
    am.same(est["retired_error"], d_err, "retired_error against the derivation")
    tc.same_state((col, cnt, px), (d_col, d_cnt, d_px), f"{scene}: frame against the unmasked states at retired_at")
    if passes is not None:
        assert est["passes"] == passes and est["pixel_passes"] == pixel_passes
    if retired_at is not None:
        assert est["retired_at"].tolist() == retired_at
    return est


def test_adaptive_render_until_cornell():
    _check_adaptive("cornell", 0.05, 384, 480864, CORNELL_RETIRED_AT)


def test_adaptive_render_until_cornell_glass():
    _check_adaptive("cornell_glass", 0.08, 448, 954584)


def test_adaptive_min_passes():
    base = tc.adaptive_run(CPU, "cornell", 0.05)[0]["retired_at"]
    est = _check_adaptive("cornell", 0.05, None, None, min_passes=128)
    early = base < 128
    assert early.any()
    assert (est["retired_at"][~early] == base[~early]).all() and (est["retired_at"][early] >= 128).all()


def test_not_adaptive_is_unchanged():
    a = g.SmallPT(64, 48, tc.scene_path("cornell"), device=CPU)
    b = g.SmallPT(64, 48, tc.scene_path("cornell"), device=CPU)
    try:
        ea = a.RenderUntil(threshold=0.2, batch=8, adaptive=False)
        # today's loop, written out
        while True:
            b.IdleFunc(8)
            eb = b.renderer.noise_estimate(threshold=0.2, remark=True)
            if nc.converged(eb) or b.current_sample >= 4096:
                break
        assert set(ea) == set(eb) | {"passes", "converged"} and ea["passes"] == b.current_sample
        for k in eb:
            assert np.array_equal(ea[k], eb[k]), k
        tc.same_state(a.colors() + (a.pixels(),), b.colors() + (b.pixels(),), "adaptive=False")
    finally:
        a.FreeBuffers()
        b.FreeBuffers()


def test_smallpt_adaptive_writes_the_same_ppm(tmp_path):
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    out = tmp_path / "c.ppm"
    r = subprocess.run([exe, "64", "48", tc.scene_path("cornell"), "--device", "-1", "--until", "0.05", "--adaptive",
                        "--batch", "8", "--out", str(out), "--dat", os.path.join(REPO, "assets", "data", "MersenneTwister.dat")],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stderr.splitlines() if l.startswith("Until 0.05 adaptive:")]
    assert len(line) == 1 and "384 passes" in line[0] and "converged" in line[0], r.stderr
    assert "480864 pixel-passes of 1223040" in line[0], line[0]
    est, col, cnt, px = tc.adaptive_run(CPU, "cornell", 0.05)
    want = tmp_path / "py.ppm"
    g.save_ppm(str(want), px)
    assert out.read_bytes() == want.read_bytes()
