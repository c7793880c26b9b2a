"""Shared by tests/test_denoise_noise_cpu.py and tests/test_gpu_denoise_noise.py (not a test module):
the numpy float32 statement of the noise-guided denoiser's definition (include/bdpt.h
bdpt_denoise_noise) in np_denoise's structure -- vectorised over the pixels with a loop
over the 25 taps -- the frames and the sweep the tests filter, and the checks both backends share.
Every comparison is on the bits of the float32 values; there is no tolerance."""
import itertools
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import bits, same, scene, schedule
from conftest import SCENES
from denoise_common import FRAMES, H5, _dot, eligible, np_denoise, to_rgba
from noise_common import big_case, case

F = np.float32
CPU = -1
EPS = F(1e-12)                                             # BDPT_DENOISE_NOISE_EPS
DEFAULTS = dict(levels=4, normal_power=5, sigma_color=0.5, noise_sigma=1.0, materials="diffuse")
# levels 1, 3, 5 x both materials x normal_power 0, 5 x noise_sigma 0.5, 1, 4
SWEEP = [dict(levels=l, materials=m, normal_power=n, noise_sigma=s)
         for l, m, n, s in itertools.product((1, 3, 5), ("diffuse", "all"), (0, 5), (0.5, 1.0, 4.0))]
# the synthetic frames: (scene of the guides, W, H) -- 7x5 lies outside the later levels' steps, 33x25
# and 65x49 cross tile and halo borders of both level kernels and of the prefilter
SYNTHETIC = [("cornell", 7, 5), ("cornell", 33, 25), ("cornell_glass", 65, 49)]


def raw_variance(colors, counter, mc, mn):
    """Part 1: v = e2(B - A) * (a / (n - a)) where the mark is valid as for bdpt_noise_estimate, -1
    where the pixel has no estimate.  mc = mn = None: no mark stored."""
    B = np.asarray(colors, F)
    if mn is None:
        return np.full(B.shape[:2], F(-1), F)
    A = np.asarray(mc, F)
    n, m = np.asarray(counter).astype(np.int64), np.asarray(mn).astype(np.int64)
    valid = (m > 0) & (n > m) & (2 * (n - m) >= m)
    with np.errstate(all="ignore"):
        a, nf = m.astype(F), n.astype(F)
        d = B - A
        v = _dot(d, d) * (a / (nf - a))
    assert v.dtype == F
    return np.where(valid, v, F(-1)).astype(F)


def _windows(Hh, Ww, dy, dx):
    y0, y1 = max(0, -dy), min(Hh, Hh - dy)
    x0, x1 = max(0, -dx), min(Ww, Ww - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def prefilter(v, ids, elig):
    """Part 2: the h-weighted mean of the estimates of the 5x5 neighbours (step 1) on the centre's
    sphere; -1 where no tap counted; an ineligible pixel keeps its raw value."""
    Hh, Ww = ids.shape
    sv, sh = np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F)
    any_tap = np.zeros((Hh, Ww), bool)
    with np.errstate(all="ignore"):
        for j in range(5):
            for i in range(5):
                win = _windows(Hh, Ww, j - 2, i - 2)
                if win is None:
                    continue
                P, Q = win
                used = elig[P] & (ids[Q] == ids[P]) & ~(v[Q] < 0)
                hw = H5[j] * H5[i]
                sv[P] = np.where(used, sv[P] + hw * v[Q], sv[P])
                sh[P] = np.where(used, sh[P] + hw, sh[P])
                any_tap[P] |= used
        vb = sv / sh
    assert vb.dtype == F
    return np.where(elig, np.where(any_tap, vb, F(-1)), v).astype(F)


def np_denoise_noise(colors, counter, mark, ids, normals, refl, levels=4, normal_power=5, sigma_color=0.5,
                     noise_sigma=1.0, materials="diffuse"):
    """The definition, in float32 and in its operation order.  mark = (mc, mn) or None (none stored).
    -> (colours [H, W, 3], carried variance [H, W], -1 where there is none)."""
    cur = np.ascontiguousarray(colors, F).copy()
    ids = np.asarray(ids)
    normals = np.ascontiguousarray(normals, F)
    Hh, Ww = ids.shape
    elig = eligible(ids, refl, materials)
    mc, mn = mark if mark is not None else (None, None)
    var = prefilter(raw_variance(colors, counter, mc, mn), ids, elig)
    with np.errstate(all="ignore"):
        isc0 = F(1.0) / (F(sigma_color) * F(sigma_color))
        s2 = F(noise_sigma) * F(noise_sigma)
        for k in range(levels):
            s = 1 << k
            isc = isc0 * F(4 ** k)
            sw = np.zeros((Hh, Ww), F)
            sv = np.zeros((Hh, Ww), F)
            sc = np.zeros((Hh, Ww, 3), F)
            has = ~(var < 0)
            for j in range(5):
                for i in range(5):
                    win = _windows(Hh, Ww, (j - 2) * s, (i - 2) * s)
                    if win is None:
                        continue
                    P, Q = win
                    used = elig[P] & (ids[Q] == ids[P])
                    d = _dot(normals[P], normals[Q])
                    wn = np.where(d > 0, d, F(0))
                    for _ in range(normal_power):
                        wn = wn * wn
                    dc = cur[Q] - cur[P]
                    e2 = _dot(dc, dc)
                    both = has[P] & has[Q]
                    t = s2 * (var[P] + var[Q]) + EPS
                    wc = np.where(both, t * (F(1) / (t + e2)), F(1) / (F(1) + e2 * isc))
                    w = ((H5[j] * H5[i]) * wn) * wc
                    assert w.dtype == F
                    vq = np.where(has[Q], var[Q], var[P])
                    sw[P] = np.where(used, sw[P] + w, sw[P])
                    sc[P] = np.where(used[..., None], sc[P] + w[..., None] * cur[Q], sc[P])
                    sv[P] = np.where(used & has[P], sv[P] + (w * w) * vq, sv[P])
            r = F(1) / sw
            out = sc * r[..., None]
            vout = (sv * r) * r
            assert out.dtype == F and vout.dtype == F
            cur = np.where(elig[..., None], out, cur)
            var = np.where(elig & has, vout, var).astype(F)
    return cur, var


def guides(name, W, H):
    """(camera, spheres, id, normal) of a scene's unjittered first hit, from the CPU backend."""
    cam, sp = scene(name, W, H)
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        aov = r.render_aov()
    return cam, sp, aov["id"], aov["normal"]


def rendered_marked(device, name, W, H, before=4, after=4):
    """(camera, spheres, colors, counter, (mc, mn)) after `before` passes, a mark and `after` more."""
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(before + after)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        r.path_passes(sid[:before], vlp[:before])
        r.noise_mark()
        r.path_passes(sid[before:], vlp[before:])
        col, cnt = r.read_radiance()
        mark = r.noise_read_mark()
    return cam, sp, col, cnt, mark


def run(r, **prm):
    """denoise_noise with every output: (colours, rgba, variance)."""
    return r.denoise_noise(pixels=True, variance=True, **prm)


def assert_matches_numpy(r, col, cnt, mark, ids, nrm, refl, what, sweep=SWEEP):
    """The renderer holds (col, cnt, mark): every output over the sweep equals the statement."""
    for prm in sweep:
        out, px, var = run(r, **prm)
        want, wvar = np_denoise_noise(col, cnt, mark, ids, nrm, refl, **prm)
        assert not np.isnan(want).any() and not np.isnan(wvar).any(), "the cases are meant to form no NaN"
        same(out, want, f"{what} {prm}: colours")
        same(var, wvar, f"{what} {prm}: variance")
        assert np.array_equal(px, to_rgba(out)), f"{what} {prm}: pixels"


def assert_equals_plain_denoise(device, name="cornell_glass", W=65, H=49):
    """Consequence 4: no mark, a cleared mark and a mark that is valid nowhere give bdpt_denoise's bits
    (and no variance anywhere) whatever noise_sigma says."""
    cam, sp, col, cnt, mark = rendered_marked(device, name, W, H)
    prms = [dict(levels=4, normal_power=5, sigma_color=0.5, materials="diffuse"),
            dict(levels=2, normal_power=0, sigma_color=0.125, materials="all")]

    def check(r, what):
        for prm in prms:
            plain, ppx = r.denoise(pixels=True, **prm)
            out, px, var = run(r, noise_sigma=3.0, **prm)
            same(out, plain, f"{what}: colours")
            assert np.array_equal(px, ppx), f"{what}: pixels"
            assert (var == F(-1)).all(), f"{what}: a variance without an estimate"

    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        check(r, "no mark stored")
        r.noise_write_mark(*mark)
        assert (run(r)[2] >= 0).any()
        r.noise_clear()
        check(r, "after noise_clear")
        # valid nowhere: the mark's count equals the frame's (no fresh samples), or 0
        y, x = np.mgrid[0:H, 0:W]
        r.noise_write_mark(mark[0], np.where((x + y) % 2, cnt, 0).astype(np.uint32))
        check(r, "a mark that is valid nowhere")


def assert_zero_variance_passes_through(device, name="cornell", W=65, H=49):
    """A mark that equals the frame with fewer samples (m < n, 2(n - m) >= m) says the variance is
    zero everywhere, so every colour difference is an edge and the frame passes through.  The bound
    the definition implies: v = 0 gives t = eps, stays 0 through the prefilter and every level (sums
    of w^2 * 0), so a tap at colour distance x = sqrt(e2) has wc = eps / (eps + x^2) and pulls the
    centre by at most x * wc <= sqrt(eps) / 2 per channel (the maximum of x eps / (eps + x^2), at
    x = sqrt(eps)), times its share of the weights.  The centre tap has wn = |n|^(2^np) and wc = 1 to
    rounding, h h = 9/64; the other taps' h h sum to 55/64 and their wn <= 1: one level moves a channel
    by at most (55/9) sqrt(eps)/2 (1 + 1e-3) = 3.06e-6, L levels by L times that (the colours a level
    reads have moved, the argument does not care).  On top comes the rounding of the 25-term weighted
    mean, at most 32 ulp of the largest colour per level."""
    cam, sp, col, cnt, _ = rendered_marked(device, name, W, H)
    cnt = np.full_like(cnt, 8)
    half = np.full_like(cnt, 4)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(col, half)
        for levels in (1, 4, 8):
            out, _, var = run(r, levels=levels, materials="all")
            assert (var == 0).all()
            bound = levels * ((55.0 / 9.0) * float(np.sqrt(EPS)) / 2 * 1.001 + 32 * 2.0 ** -24 * float(np.abs(col).max()))
            err = float(np.abs(out.astype(np.float64) - col).max())
            print(f"zero variance, {levels} levels: max |out - in| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            assert not np.array_equal(out, r.denoise(levels=levels, materials="all"))


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_denoise_noise / bdpt_last_denoise_noise_ms."""
    import ctypes
    EINVAL, ESTATE = g._lib.BDPT_EINVAL, g._lib.BDPT_ESTATE
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, device=device) as r:
        with pytest.raises(g.BdptError) as e:               # no camera yet
            r.denoise_noise()
        assert e.value.code == ESTATE
        with pytest.raises(g.BdptError) as e:
            r.last_denoise_noise_ms()
        assert e.value.code == ESTATE
        r.set_camera(cam)
        for bad in (dict(levels=0), dict(levels=9), dict(normal_power=-1), dict(normal_power=7),
                    dict(sigma_color=0.0), dict(sigma_color=float("nan")), dict(noise_sigma=0.0),
                    dict(noise_sigma=-1.0), dict(noise_sigma=float("nan")), dict(noise_sigma=float("inf"))):
            with pytest.raises(g.BdptError) as e:
                r.denoise_noise(**bad)
            assert e.value.code == EINVAL, bad
        with pytest.raises(g.BdptError) as e:
            r.last_denoise_noise_ms()
        assert e.value.code == ESTATE                        # the failed calls do not count
        col = np.empty((19, 20, 3), F)
        var = np.empty((19, 20), F)
        ptr, vptr = ctypes.c_void_p(col.ctypes.data), ctypes.c_void_p(var.ctypes.data)
        prm = g._lib.DenoiseNoiseParams(4, 5, 0.5, 0, 1.0)
        call = g.lib.bdpt_denoise_noise
        assert call(r._h, ctypes.byref(prm), None, None, None) == EINVAL       # both outputs NULL
        assert call(r._h, ctypes.byref(prm), None, None, vptr) == EINVAL       # the variance alone is none
        assert call(r._h, None, ptr, None, None) == EINVAL                     # no parameters
        for m in (2, -1):
            assert call(r._h, ctypes.byref(g._lib.DenoiseNoiseParams(4, 5, 0.5, m, 1.0)), ptr, None, None) == EINVAL
        assert call(None, ctypes.byref(prm), ptr, None, None) == EINVAL
        # valid at the ends of every range; a frame that was never rendered is all zeros and stays so
        out, px, v = run(r, levels=8, normal_power=6, sigma_color=float("inf"), noise_sigma=1e-10, materials="all")
        assert (bits(out) == 0).all() and not px.any() and (v == F(-1)).all()
        assert r.last_denoise_noise_ms() >= 0.0
        with pytest.raises(g.BdptError) as e:                # the plain denoiser's clock is its own
            r.last_denoise_ms()
        assert e.value.code == ESTATE


def assert_non_interference(device, name, W, H, streams=None):
    """4 passes, mark, 2 passes, denoise_noise (defaults and an 8-level one with every output), 2 passes
    == the same without the calls: frame, counters, pixels, table, light paths and the mark; on the GPU
    the calls are queued behind unsynchronised passes, and what they filtered was the finished frame."""
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(8)
    got, mid = [], []
    for probe in (False, True):
        with g.Renderer(sp, W, H, cam, device=device) as r:
            if streams is not None:
                r.set_streams(streams)
            r.light_pass(0)
            r.path_passes(sid[:4], vlp[:4])
            r.noise_mark()
            r.path_passes(sid[4:6], vlp[4:6], sync=not probe)
            if probe:
                mid.append(run(r))
                run(r, levels=8, materials="all", noise_sigma=2.0)
            r.path_passes(sid[6:], vlp[6:])
            col, cnt = r.read_radiance()
            mc, mn = r.noise_read_mark()
            got.append((col, cnt, r.read_pixels(), r.read_rand(), r.read_lightpaths(), mc, mn))
    for a, b, what in zip(got[0], got[1], ("colors", "counter", "pixels", "rand", "lightpaths", "mark colours", "mark counts")):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what
    assert (got[0][1] == 8).all() and (got[0][6] == 4).all()
    with g.Renderer(sp, W, H, cam, device=device) as r:
        if streams is not None:
            r.set_streams(streams)
        r.light_pass(0)
        r.path_passes(sid[:4], vlp[:4])
        r.noise_mark()
        r.path_passes(sid[4:6], vlp[4:6])
        col6, cnt6 = r.read_radiance()
        mark = r.noise_read_mark()
        again = run(r)
        aov = r.render_aov()
    want, wvar = np_denoise_noise(col6, cnt6, mark, aov["id"], aov["normal"], sp["refl"])
    for a, b, what in zip(mid[0], again, ("colours", "pixels", "variance")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"queued behind unsynchronised passes or not: {what}"
    same(again[0], want, "the denoised 6-pass frame vs numpy")
    same(again[2], wvar, "its variance vs numpy")


def assert_render_until(device, threshold=0.05, max_passes=48, batch=8):
    """RenderUntil(denoise=True): passes, estimate and frame are the plain call's, bit for bit, and
    r["denoised"] is denoise_noise() called by hand before any re-mark."""
    from noise_common import same_estimate
    scn = os.path.join(SCENES, "cornell.scn")
    res = []
    for dn in (False, True):
        app = g.SmallPT(64, 48, scn, device=device)
        try:
            r = app.RenderUntil(threshold=threshold, max_passes=max_passes, batch=batch, pixels=True, denoise=dn)
            res.append((r, app.colors()))
        finally:
            app.FreeBuffers()
    (plain, pf), (with_dn, df) = res
    assert "denoised" not in plain and plain["passes"] == with_dn["passes"] and plain["converged"] == with_dn["converged"]
    same_estimate(with_dn, plain, "the estimate with denoise=True")
    for a, b, what in zip(pf, df, ("colours", "counters")):
        same(a, b, f"RenderUntil(denoise=True): {what}")
    # by hand: the same IdleFunc calls, the estimates the loop makes, and the filter before the last re-mark
    app = g.SmallPT(64, 48, scn, device=device)
    try:
        while True:
            app.IdleFunc(batch)
            est = app.renderer.noise_estimate(threshold=threshold, remark=False)
            done = est["valid_pixels"] > 0 and est["pending_pixels"] == 0 and est["tiles_over"] == 0
            if done or app.current_sample >= max_passes:
                break
            app.renderer.noise_estimate(threshold=threshold, remark=True)
        hand = app.renderer.denoise_noise()
        assert (app.renderer.denoise_noise(variance=True)[1] >= 0).any(), "no estimate left for the filter"
    finally:
        app.FreeBuffers()
    same(with_dn["denoised"], hand, "r['denoised'] vs denoise_noise() by hand")
