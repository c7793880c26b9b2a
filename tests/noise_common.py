"""Shared by the noise-estimate tests (CPU backend and GPU): the definition of include/bdpt.h
bdpt_noise_estimate stated once more in numpy float32 -- per pixel, the tile tree, the summary and
the re-marking -- and the cases both backends are compared on.  Every comparison is on the bits."""
import functools
import os
import struct

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from conftest import SCENES
from denoise_common import synthetic_radiance

F = np.float32
CPU = -1
TW, TH = 32, 8
CAP = 30000
SUMMARY = ("valid_pixels", "pending_pixels", "tiles_x", "tiles_y", "valid_tiles", "tiles_over", "mean", "max_tile")
FRAMES = [(32, 8), (33, 9), (65, 49), (40, 33), (7, 5), (129, 3)]
COUNTS = np.array([0, 1, 2, 3, 4, 29999, 30000], np.int64)
PARAMS = [dict(dark=0.01, threshold=0.05), dict(dark=1e-3, threshold=2.0)]


def np_noise(colors, counter, mc, mn, dark=0.01, threshold=0.05, remark=False):
    """The definition: -> dict of error [H, W], tile_sum / tile_error / tile_valid / tile_pending
    [tiles_y, tiles_x], the summary's fields, and mark = (mc, mn) after the call."""
    B, A = np.asarray(colors, F), np.asarray(mc, F)
    cnt, m = np.asarray(counter).astype(np.int64), np.asarray(mn).astype(np.int64)
    H, W = cnt.shape
    valid = (m > 0) & (cnt > m) & (2 * (cnt - m) >= m)
    with np.errstate(all="ignore"):
        a, n = m.astype(F), cnt.astype(F)
        d = B - A
        e1 = (np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2])
        s = a / (n - a)
        f = np.sqrt(s)
        lum = (B[..., 0] + B[..., 1]) + B[..., 2]
        den = np.sqrt(np.fmax(lum, F(dark)))
        e = (e1 * f) / den
    assert e.dtype == F
    error = np.where(valid, e, F(-1.0)).astype(F)
    growing = (cnt > 0) & (cnt < CAP)
    pending = growing & ~valid
    ty, tx = -(-H // TH), -(-W // TW)

    def tiles(plane):
        pad = np.zeros((ty * TH, tx * TW), plane.dtype)
        pad[:H, :W] = plane
        return pad.reshape(ty, TH, tx, TW).transpose(0, 2, 1, 3).reshape(ty, tx, TH * TW)

    v = tiles(np.where(valid, e, F(0.0)).astype(F))
    with np.errstate(all="ignore"):
        for _ in range(8):
            v = v[..., 0::2] + v[..., 1::2]
    S = v[..., 0].astype(F)
    c = tiles(valid.astype(np.uint32)).sum(axis=2).astype(np.uint32)
    p = tiles(pending.astype(np.uint32)).sum(axis=2).astype(np.uint32)
    with np.errstate(all="ignore"):
        E = np.where(c > 0, S / np.maximum(c, 1).astype(F), F(0.0)).astype(F)
    total, worst = 0.0, F(0.0)
    for t in range(ty * tx):                              # row-major, in doubles, one after the other
        total += float(S.ravel()[t])
        if E.ravel()[t] > worst:
            worst = E.ravel()[t]
    nv = int(c.sum())
    out = dict(error=error, tile_sum=S, tile_error=E, tile_valid=c, tile_pending=p, valid_pixels=nv,
               pending_pixels=int(p.sum()), tiles_x=tx, tiles_y=ty, valid_tiles=int((c > 0).sum()),
               tiles_over=int((E > F(threshold)).sum()), mean=total / nv if nv else 0.0, max_tile=float(worst))
    mc2, mn2 = A.copy(), np.asarray(mn).astype(np.uint32).copy()
    if remark:
        take = growing & (cnt >= 2 * m)
        mc2[take] = B[take]
        mn2[take] = cnt[take].astype(np.uint32)
    out["mark"] = (mc2, mn2)
    return out


def converged(est):
    return est["valid_pixels"] > 0 and est["pending_pixels"] == 0 and est["tiles_over"] == 0


def same_summary(got, want, what):
    for k in SUMMARY:
        if k == "mean":
            assert struct.pack("<d", got[k]) == struct.pack("<d", want[k]), f"{what}: mean {got[k]!r} vs {want[k]!r}"
        elif k == "max_tile":
            assert struct.pack("<f", got[k]) == struct.pack("<f", want[k]), f"{what}: max_tile {got[k]!r} vs {want[k]!r}"
        else:
            assert got[k] == want[k], f"{what}: {k} {got[k]} vs {want[k]}"


def same_estimate(got, want, what):
    """Two results (a backend's run_case or np_noise) agree on every bit they both hold."""
    for k in ("error", "tile_error", "tile_valid"):
        same(got[k], want[k], f"{what}: {k}")
    same_summary(got, want, what)
    if "mark" in got and "mark" in want:
        same(got["mark"][0], want["mark"][0], f"{what}: mark colours")
        same(got["mark"][1], want["mark"][1], f"{what}: mark counts")


@functools.lru_cache(maxsize=None)
def case(W, H):
    """Colours and mark colours of seeded values with 0, -0, 1e-30 and 1e18; counters from COUNTS;
    marks patterned per pixel over {0, cnt, cnt-1, ceil(2cnt/3), ceil(2cnt/3)-1, cnt/2, cnt+5}: the
    fresh-sample rule 3 mn <= 2 cnt is met on both sides of its boundary.  Where the frame has them,
    tile (0, 0) is made all valid and tile (1, 0) is left without a mark."""
    rng = np.random.default_rng(100 * W + H)
    col, mc = synthetic_radiance(W, H, seed=5), synthetic_radiance(W, H, seed=7)
    cnt = COUNTS[rng.integers(0, len(COUNTS), (H, W))]
    y, x = np.mgrid[0:H, 0:W]
    top = -(-2 * cnt // 3)
    pats = np.stack([0 * cnt, cnt, cnt - 1, top, top - 1, cnt // 2, cnt + 5])
    mn = np.maximum(np.take_along_axis(pats, ((x + 3 * y) % 7)[None], 0)[0], 0)
    if W >= TW and H >= TH:
        cnt[:TH, :TW] = COUNTS[2:][rng.integers(0, len(COUNTS) - 2, (TH, TW))]
        mn[:TH, :TW] = cnt[:TH, :TW] // 2
    if W > TW:
        mn[:TH, TW:2 * TW] = 0
    for a in (col, mc):
        a.setflags(write=False)
    return col, cnt.astype(np.uint32), mc, mn.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def big_case(W=40, H=33):
    """Counts and marks near 2^31 and 2^32, where 2*(cnt - mn) and 2*mn do not fit 32 bits, around
    the fresh-sample boundary, next to small counts that take the mark."""
    col, _, mc, _ = case(W, H)
    y, x = np.mgrid[0:H, 0:W]
    cnt = np.array([0xfffffff0, 0x80000001, 0x80000000, 0x7fffffff, 3, 29999], np.int64)[(x + y) % 6]
    top = -(-2 * cnt // 3)
    pats = np.stack([cnt // 2, top, top - 1, cnt - 1, (cnt + 1) // 2, cnt // 2 + 1, 0 * cnt + 1])
    mn = np.take_along_axis(pats, ((x + 3 * y) % 7)[None], 0)[0]
    return col, cnt.astype(np.uint32), mc, mn.astype(np.uint32)


def run_case(device, W, H, remark, **prm):
    """The case of frame W x H on a backend: the estimate with the per-pixel plane and the mark
    read back afterwards."""
    return run_arrays(device, *case(W, H), remark, **prm)


def run_arrays(device, col, cnt, mc, mn, remark, **prm):
    H, W = cnt.shape
    cam, sp = scene("cornell", W, H)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(mc, mn)
        out = r.noise_estimate(remark=remark, pixels=True, **prm)
        out["mark"] = r.noise_read_mark()
        frame = r.read_radiance()
        same(frame[0], col, "the accumulation is only read")
        same(frame[1], cnt, "the counters are only read")
        again = r.noise_estimate(remark=False, pixels=True, **prm)
    if not remark:
        same_estimate(again, out, f"{W}x{H}: a second call")
    return out


def want_case(W, H, remark, **prm):
    col, cnt, mc, mn = case(W, H)
    return np_noise(col, cnt, mc, mn, remark=remark, **prm)


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_noise_*."""
    import ctypes
    W, H = 33, 9
    cam, sp = scene("cornell", W, H)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        for call in (r.noise_read_mark, r.last_noise_ms):
            with pytest.raises(g.BdptError) as ei:
                call()
            assert ei.value.code == g._lib.BDPT_ESTATE
        bad = [dict(dark=0.0), dict(dark=-1.0), dict(dark=float("nan")), dict(threshold=-0.5), dict(threshold=float("nan"))]
        for prm in bad:
            with pytest.raises(g.BdptError) as ei:
                r.noise_estimate(**prm)
            assert ei.value.code == g._lib.BDPT_EINVAL, prm
        prm = g._lib.NoiseParams(0.01, 0.05, 0)
        sm = g._lib.NoiseSummary()
        lib = g.lib
        assert lib.bdpt_noise_estimate(r._h, None, None, None, None, ctypes.byref(sm)) == g._lib.BDPT_EINVAL
        assert lib.bdpt_noise_estimate(r._h, ctypes.byref(prm), None, None, None, None) == g._lib.BDPT_EINVAL
        with pytest.raises(g.BdptError) as ei:                # after failures only: still no estimate
            r.last_noise_ms()
        assert ei.value.code == g._lib.BDPT_ESTATE
        assert lib.bdpt_noise_estimate(r._h, ctypes.byref(prm), None, None, None, ctypes.byref(sm)) == g.BDPT_OK
        assert sm.valid_pixels == 0 and (sm.tiles_x, sm.tiles_y) == (2, 2) == r.noise_tiles()
        assert r.last_noise_ms() >= 0.0
        with pytest.raises(g.BdptError) as ei:                # an estimate without remark stores no mark
            r.noise_read_mark()
        assert ei.value.code == g._lib.BDPT_ESTATE
        r.noise_estimate(threshold=0.0, dark=float("inf"))    # both allowed


def rendered_pair(device, passes_a, passes_b, W=64, H=48, name="cornell"):
    """SmallPT(W, H, name): passes_a passes, mark, passes_b more, estimate -> (estimate with the
    per-pixel plane, the frame's colours)."""
    app = g.SmallPT(W, H, os.path.join(SCENES, name + ".scn"), device=device)
    try:
        app.IdleFunc(passes_a)
        app.renderer.noise_mark()
        app.IdleFunc(passes_b)
        est = app.renderer.noise_estimate(pixels=True)
        return est, app.colors()[0]
    finally:
        app.FreeBuffers()


def np_render_until(device, threshold, max_passes, batch, W=64, H=48, name="cornell", dark=0.01):
    """What RenderUntil must do, from outside: a SmallPT that makes the same IdleFunc(batch) calls
    and no noise call, its frames read back and the numpy statement driven over them with a mark
    of its own.  -> (the last estimate with passes and converged, colours, counters)."""
    app = g.SmallPT(W, H, os.path.join(SCENES, name + ".scn"), device=device)
    try:
        mc = np.zeros((app.height, app.width, 3), F)
        mn = np.zeros((app.height, app.width), np.uint32)
        while True:
            app.IdleFunc(batch)
            col, cnt = app.colors()
            est = np_noise(col, cnt, mc, mn, dark=dark, threshold=threshold, remark=True)
            mc, mn = est["mark"]
            if converged(est) or app.current_sample >= max_passes:
                break
        est["passes"], est["converged"] = app.current_sample, converged(est)
        return est, col, cnt
    finally:
        app.FreeBuffers()
