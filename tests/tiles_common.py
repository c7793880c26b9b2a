"""Shared by the tile-mask tests (tests/test_tiles_cpu.py, tests/test_gpu_tiles.py; not a test
module): the masks, what a masked call must leave -- the oracle's *unmasked* result from the same
state, chosen per pixel by the mask, else the state before the call -- and the adaptive RenderUntil
stated once more on an unmasked render and the numpy noise estimate.  Every comparison is on bits."""
import functools
import os

import numpy as np

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g
import oracle
from conftest import SCENES
from noise_common import np_noise

W, H = am.W, am.H                   # 97 x 65: 4 x 9 tiles, the last column 1 pixel wide, the last row 1 high
TW, TH = 32, 8
TX, TY = -(-W // TW), -(-H // TH)


def mask(name, tx=TX, ty=TY):
    """A: checkerboard with the corner tile; B: the last column, the last row and one interior tile
    (the pixels an unmasked launch packs); C: tile (0, 0) alone; Z: none; F: all."""
    y, x = np.mgrid[0:ty, 0:tx]
    if name == "A":
        m = (x + y) % 2 == (tx - 1 + ty - 1) % 2
        assert m[ty - 1, tx - 1]
    elif name == "B":
        m = (x == tx - 1) | (y == ty - 1)
        m[ty // 2, min(1, tx - 1)] = True
    elif name == "C":
        m = (x == 0) & (y == 0)
    elif name == "Z":
        m = np.zeros((ty, tx), bool)
    else:
        assert name == "F"
        m = np.ones((ty, tx), bool)
    return m.astype(np.uint8)


def pixel_mask(tiles, width, height):
    return np.repeat(np.repeat(np.asarray(tiles) != 0, TH, 0), TW, 1)[:height, :width]


def tile_pixels(tiles, width, height):
    return int(pixel_mask(tiles, width, height).sum())


_CHAIN = {}


def chain(scene, state0, steps, width=W, height=H):
    """The states after the calls `steps` = ((mask name, passes), ...) from state0 = (colors, counter,
    pixels) after light_pass(0): per call the oracle's unmasked passes from the state before it,
    taken where the mask says and the state before elsewhere.  Computed once per input."""
    key = (scene, steps, width, height) + tuple(np.ascontiguousarray(a).tobytes() for a in state0)
    if key in _CHAIN:
        return _CHAIN[key]
    sc = am.Scenario("tiles", scene, (), width=width, height=height)
    cam, sp = am.load_scene(sc)
    rnd = oracle.mt607(0)
    lp = oracle.light_pass(sp, rnd, 0)
    sid, vlp = am.schedule(sum(n for _, n in steps))
    col, cnt, px = (np.array(a) for a in state0)
    out, p = [], 0
    for name, n in steps:
        ocol, ocnt, opx = oracle.path_passes(sp, rnd, cam, width, height, lp, sid[p:p + n], vlp[p:p + n],
                                             colors=col.copy(), counter=cnt.copy(), pixels=px.copy())
        m = pixel_mask(mask(name, -(-width // TW), -(-height // TH)), width, height)
        col = np.where(m[..., None], ocol, col)
        cnt = np.where(m, ocnt, cnt)
        px = np.where(m[..., None], opx, px)
        p += n
        out.append((col, cnt, px))
    _CHAIN[key] = out
    return out


def same_state(got, want, what):
    for a, b, k in zip(got, want, ("colors", "counter", "pixels")):
        am.same(a, b, f"{what}: {k}")


def read_state(r):
    col, cnt = r.read_radiance()
    return col, cnt, r.read_pixels()


def masked_call(r, mode, sid, vlp, limit, tiles):
    """One masked path_passes call in `mode` (None: the CPU backend) with the proof of what ran, as
    accum_modes._call proves it for an unmasked call, plus the tile list and no pools or units."""
    n = len(sid)
    if mode is None:
        r.path_passes(sid, vlp, tiles=tiles)
        return
    fused = mode.last_streams(n) == 1
    L, launches = am.launch_passes(n, limit, fused)
    assert L >= mode.min_launch
    r.set_streams(n if mode.streams is None else mode.streams)
    if mode.choice is not None:
        r.set_stream_choice(mode.choice)
    r.kernel_timing(reset=True)
    r.path_passes(sid, vlp, tiles=tiles)
    what = f"{mode.name}: masked call of {n} passes, limit {limit}"
    assert r.kernel_timing(reset=True)[1] == launches, f"{what}: not {launches} launches"
    assert r.last_streams == mode.last_streams(L), f"{what}: last_streams {r.last_streams}"
    if mode.choice is not None:
        assert r.stream_choice == mode.choice, f"{what}: stream_choice {r.stream_choice:#x}"
    assert "tile_list" in r.last_features, f"{what}: {r.last_features}"
    for other in ("pixel_pools", "unit_fold"):
        assert other not in r.last_features, f"{what}: {r.last_features}"
    assert r.last_specialized == mode.specialize, f"{what}: specialised {r.last_specialized}: {r.specialize_status!r}"
    assert r.last_traversal == ("bvh" if mode.bvh else "brute"), f"{what}: {r.last_traversal}"


def run_masked(mode, scene, steps, device, monkeypatch=None, limit=None):
    """write_radiance(uneven_state(W, H, 7)) after light_pass(0), then the masked calls `steps`;
    -> (state0, [state after every call])."""
    if mode is not None:
        am.force_env(mode, limit, monkeypatch)
    sc = am.Scenario("tiles", scene, ())
    cam, sp = am.load_scene(sc)
    sid, vlp = am.schedule(sum(n for _, n in steps))
    out, p = [], 0
    with g.Renderer(sp, W, H, cam, device=device) as r:
        if mode is not None:
            r.set_specialize(mode.specialize)
            if mode.bvh:
                assert r.has_bvh
                r.set_traversal("bvh")
        r.light_pass(0)
        r.write_radiance(*am.uneven_state(W, H, 7))
        state0 = read_state(r)
        for name, n in steps:
            masked_call(r, mode, sid[p:p + n], vlp[p:p + n], limit, mask(name))
            p += n
            out.append(read_state(r))
    return state0, out


def check_masked(mode, scene, steps, device, monkeypatch=None, limit=None):
    state0, got = run_masked(mode, scene, steps, device, monkeypatch, limit)
    want = chain(scene, state0, steps)
    done = 0
    for k, (name, n) in enumerate(steps):
        done += n
        same_state(got[k], want[k], f"{mode.name if mode else 'cpu'} {scene}: after call {k + 1} (mask {name}, {done} passes)")


# ---- adaptive RenderUntil -------------------------------------------------------------------------

def scene_path(name):
    return os.path.join(SCENES, name + ".scn")


@functools.lru_cache(maxsize=None)
def adaptive_run(device, scene, threshold, min_passes=0, batch=8):
    """RenderUntil(adaptive=True) of SmallPT(64, 48, scene) on `device` -> (result dict, colors,
    counter, pixels)."""
    app = g.SmallPT(64, 48, scene_path(scene), device=device)
    try:
        est = app.RenderUntil(threshold=threshold, batch=batch, adaptive=True, min_passes=min_passes)
        col, cnt = app.colors()
        return est, col, cnt, app.pixels()
    finally:
        app.FreeBuffers()


@functools.lru_cache(maxsize=None)
def adaptive_derived(scene, threshold, min_passes=0, batch=8, max_passes=4096):
    """The same loop stated on an unmasked CPU render: IdleFunc(batch) on every pixel, and per check
    the numpy estimate of the frame each tile would hold -- a retired tile's pixels stay at their
    state of retired_at, so the estimate runs on a frame composed per tile, with a mark kept here.
    -> (retired_at, retired_error, pixel_passes, passes, colors, counter, pixels of the composed frame)."""
    app = g.SmallPT(64, 48, scene_path(scene), device=-1)
    try:
        Wf, Hf = app.width, app.height
        tx, ty = -(-Wf // TW), -(-Hf // TH)
        retired_at = np.zeros((ty, tx), np.int32)
        retired_error = np.zeros((ty, tx), np.float32)
        col = np.zeros((Hf, Wf, 3), np.float32)
        cnt = np.zeros((Hf, Wf), np.uint32)
        px = np.zeros((Hf, Wf, 4), np.uint8)
        mc, mn = np.zeros_like(col), np.zeros_like(cnt)
        pixel_passes = 0
        while True:
            live = retired_at == 0
            app.IdleFunc(batch)
            pixel_passes += batch * tile_pixels(live, Wf, Hf)
            m = pixel_mask(live, Wf, Hf)
            ucol, ucnt = app.colors()
            upx = app.pixels()
            col, cnt, px = np.where(m[..., None], ucol, col), np.where(m, ucnt, cnt), np.where(m[..., None], upx, px)
            est = np_noise(col, cnt, mc, mn, threshold=threshold, remark=True)
            mc, mn = est["mark"]
            settled = (est["tile_valid"] == 0) | (est["tile_error"] <= np.float32(threshold))
            retire = live & (est["tile_pending"] == 0) & settled & (app.current_sample >= min_passes)
            retired_at[retire] = app.current_sample
            retired_error[retire] = est["tile_error"][retire]
            if (retired_at != 0).all() or app.current_sample >= max_passes:
                break
        return retired_at, retired_error, pixel_passes, app.current_sample, col, cnt, px
    finally:
        app.FreeBuffers()
