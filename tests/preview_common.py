"""Shared by tests/test_preview_denoise_cpu.py and tests/test_gpu_preview_denoise.py (not a test
module): the numpy float32 statement of the denoised preview (include/bdpt.h bdpt_preview_denoise,
DESIGN.md 4f) -- np_reproject's (out, tot) through the count-weighted a-trous levels, vectorised over
the pixels with a loop over the 25 taps -- the parameter sets the tests run, and the checks both
backends share.  Every comparison of a backend with the statement or with the other backend is on
the bits of the float32 values; there is no tolerance."""
import ctypes
import functools

import numpy as np

import gpu_bidirectional_raytracer_amd as g
from aov_common import bits, same, scene, schedule
from denoise_common import H5, eligible, rendered_frame, synthetic_radiance, to_rgba
from reproject_common import (CPU, F, FRAMES, INF, MOVES, _dot, case_of, first_hit, hist_dict, history_of, moved,
                              np_reproject, rendered)

DEFAULTS = dict(levels=4, normal_power=5, sigma_color=0.5, count_ref=8.0, max_history=64.0, plane_tol=0.01,
                materials="diffuse")
LO, HI = F(2.0 ** -20), F(2.0 ** 40)


def _p(levels, materials, normal_power, sigma_color, count_ref, max_history):
    return dict(levels=levels, materials=materials, normal_power=normal_power, sigma_color=sigma_color,
                count_ref=count_ref, max_history=max_history)


# every value of levels 0, 1, 3, 5 x both materials x normal_power 0, 5, 6 x sigma_color 0.5, 1e-3,
# inf x count_ref 1, 8, 100 x max_history 2, 64, inf occurs, each with at least two partners
PARAMS = [_p(0, "diffuse", 5, 0.5, 8.0, 64.0), _p(0, "all", 0, 1e-3, 1.0, INF),
          _p(1, "all", 0, 1e-3, 1.0, 2.0), _p(1, "diffuse", 6, 0.5, 100.0, INF),
          _p(3, "diffuse", 6, INF, 100.0, INF), _p(3, "all", 5, 1e-3, 8.0, 64.0),
          _p(5, "all", 5, 0.5, 8.0, 2.0), _p(5, "diffuse", 0, INF, 1.0, 64.0),
          _p(4, "diffuse", 5, 0.5, 8.0, 64.0)]
# at 7x5 every off-centre tap is outside the frame from step 8 on
PARAMS_7x5 = PARAMS + [_p(8, "all", 5, 0.5, 8.0, 64.0), _p(8, "diffuse", 6, 1e-3, 100.0, INF)]


def params_of(W, H):
    return PARAMS_7x5 if (W, H) == (7, 5) else PARAMS


def clampc(w):
    """0 when w == 0, otherwise fminf(fmaxf(w, 2^-20), 2^40) (fmin / fmax: a NaN gives the bound)."""
    w = np.asarray(w, F)
    return np.where(w == 0, F(0), np.fmin(np.fmax(w, LO), HI)).astype(F)


def np_preview_levels(o, tot, ids, normals, refl, levels, normal_power, sigma_color, count_ref, materials):
    """The levels of the definition on a frame (o, tot), in float32 and in its operation order.
    Returns (colours, counts)."""
    cur = np.ascontiguousarray(o, F).copy()
    a = np.ascontiguousarray(tot, F).copy()
    if levels == 0:
        return cur, a
    ids = np.asarray(ids)
    normals = np.ascontiguousarray(normals, F)
    Hh, Ww = ids.shape
    elig = eligible(ids, refl, materials)
    with np.errstate(all="ignore"):
        a = clampc(a)
        isc0 = F(1.0) / (F(sigma_color) * F(sigma_color))
        c2 = F(2.0) / F(count_ref)
        for k in range(levels):
            s = 1 << k
            isc = isc0 * F(4 ** k)
            su, sw = np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F)
            sc = np.zeros((Hh, Ww, 3), F)
            any_used = np.zeros((Hh, Ww), bool)
            for j in range(5):
                for i in range(5):
                    dy, dx = (j - 2) * s, (i - 2) * s
                    y0, y1 = max(0, -dy), min(Hh, Hh - dy)
                    x0, x1 = max(0, -dx), min(Ww, Ww - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    ap, aq = a[P], a[Q]
                    used = elig[P] & (ids[Q] == ids[P]) & (aq > 0)
                    d = _dot(normals[P], normals[Q])
                    wn = np.where(d > 0, d, F(0))
                    for _ in range(normal_power):
                        wn = wn * wn
                    dc = cur[Q] - cur[P]
                    e2 = _dot(dc, dc)
                    gg = ((ap * aq) * (F(1) / (ap + aq))) * c2
                    wc = np.where(ap != 0, F(1) / (F(1) + (e2 * isc) * gg), F(1))
                    u = ((H5[j] * H5[i]) * wn) * wc
                    w = u * aq
                    assert u.dtype == F and w.dtype == F and gg.dtype == F
                    su[P] = np.where(used, su[P] + u, su[P])
                    sw[P] = np.where(used, sw[P] + w, sw[P])
                    sc[P] = np.where(used[..., None], sc[P] + w[..., None] * cur[Q], sc[P])
                    any_used[P] |= used
            out = sc * (F(1) / sw)[..., None]
            cnt = clampc(sw / su)
            assert out.dtype == F and cnt.dtype == F
            cur = np.where(any_used[..., None], out, cur)
            a = np.where(any_used, cnt, a)
    return cur, a


def np_preview_denoise(colors, counter, aov, refl, hist, levels=4, normal_power=5, sigma_color=0.5, count_ref=8.0,
                       max_history=64.0, plane_tol=0.01, materials="diffuse"):
    """The definition: np_reproject's (out, tot) under (max_history, plane_tol, materials), then the
    levels.  Arguments as for np_reproject.  Returns (colours, counts, the reprojection's tot)."""
    o, tot, _ = np_reproject(colors, counter, aov, refl, hist, max_history, plane_tol, materials)
    col, a = np_preview_levels(o, tot, aov["id"], aov["normal"], refl, levels, normal_power, sigma_color, count_ref,
                               materials)
    return col, a, tot


def results(device, name, W, H, traversal, keys, hm=None):
    """preview_denoise (colours, count, rgba) over params_of(W, H): history written under the old
    camera, a one-pass frame under the new one (both rendered once on the CPU backend)."""
    cam0, sp, hc, hm4, _ = history_of(name, W, H)
    hm = hm4 if hm is None else hm
    cam1, col, cnt, _ = case_of(name, W, H, keys)
    with g.Renderer(sp, W, H, cam1, device=device) as r:
        if traversal and device != CPU:
            r.set_traversal(traversal)
        r.write_radiance(col, cnt)
        r.history_write(cam0, hc, hm)
        res = [r.preview_denoise(weight=True, pixels=True, **prm) for prm in params_of(W, H)]
        same(r.read_radiance()[0], col, "the accumulation is only read")
        same(r.history_read()[0], hc, "the history is only read: colours")
        same(r.history_read()[1], hm, "the history is only read: weight")
        if device != CPU:
            assert r.last_preview_ms() > 0.0
    return res


def block_weights(W, H):
    """0, 1e-30, 0.5, 1, 64, 3e4 and 1e30 in 4 x 4 blocks."""
    vals = np.array([0.0, 1e-30, 0.5, 1.0, 64.0, 3e4, 1e30], F)
    y, x = np.mgrid[0:H, 0:W]
    return vals[((x // 4) + 3 * (y // 4)) % 7]


SYNTHETIC = ("cornell_glass", 40, 33, ("left",))
SYNTHETIC_PARAMS = [_p(1, "all", 5, 0.5, 8.0, INF), _p(3, "diffuse", 0, 1e-3, 1.0, INF),
                    _p(5, "all", 6, INF, 100.0, 64.0), _p(4, "diffuse", 5, 0.5, 8.0, 2.0)]


@functools.lru_cache(maxsize=None)
def synthetic_inputs():
    name, W, H, keys = SYNTHETIC
    cam0, sp = scene(name, W, H)
    cam1 = moved(cam0, keys, W, H)
    col1, cnt1 = rendered(CPU, sp, W, H, cam1, 1)
    return cam0, cam1, sp, synthetic_radiance(W, H), block_weights(W, H), col1, cnt1


def synthetic_results(device):
    """[from a reset accumulation, after one pass] x SYNTHETIC_PARAMS: (colours, count, rgba)."""
    name, W, H, _ = SYNTHETIC
    cam0, cam1, sp, hc, hm, col1, cnt1 = synthetic_inputs()
    res = []
    with g.Renderer(sp, W, H, cam1, device=device) as r:
        r.history_write(cam0, hc, hm)
        for one_pass in (False, True):
            if one_pass:
                r.write_radiance(col1, cnt1)
            else:
                r.reset_accum()
            res.append([r.preview_denoise(weight=True, pixels=True, **prm) for prm in SYNTHETIC_PARAMS])
    return res


def synthetic_input_is_finite():
    """Per state and parameter set: whether the reprojected frame the levels start from is finite.
    After one pass, n >= 1 meets m = 1e30 x a colour of 1e18 where max_history does not cap the
    weight, and bdpt_reproject's own blend overflows (non-finite radiance is not special there)."""
    name, W, H, _ = SYNTHETIC
    cam0, cam1, sp, hc, hm, col1, cnt1 = synthetic_inputs()
    aov0, aov1 = first_hit(sp, W, H, cam0), first_hit(sp, W, H, cam1)
    hist = hist_dict(cam0, hc, hm, aov0)
    zero = np.zeros((H, W, 3), F), np.zeros((H, W), np.uint32)
    return [[bool(np.isfinite(np_reproject(col, cnt, aov1, sp["refl"], hist, prm["max_history"], 0.01,
                                           prm["materials"])[0]).all()) for prm in SYNTHETIC_PARAMS]
            for col, cnt in (zero, (col1, cnt1))]


def same_up_to_nan_payload(a, b, what):
    """Bit equality, except that a NaN equals any NaN: sign and payload of a NaN that an operation
    produces are not fixed by IEEE 754 and differ between the host's and the GPU's arithmetic."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaNs in different places"
    same(np.where(na, F(0), a), np.where(nb, F(0), b), what)


def assert_identity_with_denoise(device, name, W, H, normal_powers=(0, 5)):
    """No history, 8 passes everywhere, count_ref = 8: preview_denoise == denoise bit for bit, and
    the carried count is exactly 8 on eligible pixels."""
    cam, sp, col, cnt = rendered_frame(device, name, W, H, npass=8)
    assert (cnt == 8).all()
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        ids = r.render_aov()["id"]
        for levels in (1, 3, 5):
            for npow in normal_powers:
                for materials in ("diffuse", "all"):
                    what = f"{name} {W}x{H} levels {levels} normal_power {npow} {materials}"
                    want, wpx = r.denoise(levels=levels, normal_power=npow, materials=materials, pixels=True)
                    got, w, px = r.preview_denoise(levels=levels, normal_power=npow, materials=materials,
                                                   count_ref=8.0, weight=True, pixels=True)
                    same(got, want, what + ": preview_denoise vs denoise")
                    assert np.array_equal(px, wpx), what
                    e = eligible(ids, sp["refl"], materials)
                    assert e.any() and (bits(w[e]) == bits(np.full(1, 8, F))[0]).all(), what
                    assert (w[~e] == 8).all(), what


def assert_levels0_is_reproject(device, name, W, H, keys):
    from reproject_common import SWEEP
    cam0, sp, hc, hm, _ = history_of(name, W, H)
    cam1, col, cnt, _ = case_of(name, W, H, keys)
    with g.Renderer(sp, W, H, cam1, device=device) as r:
        r.write_radiance(col, cnt)
        r.history_write(cam0, hc, hm)
        for prm in SWEEP:
            a, aw, ap = r.reproject(weight=True, pixels=True, **prm)
            b, bw, bp = r.preview_denoise(levels=0, weight=True, pixels=True, **prm)
            same(b, a, f"levels=0 vs reproject {prm}: colours")
            same(bw, aw, f"levels=0 vs reproject {prm}: weight")
            assert np.array_equal(ap, bp), prm


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_preview_denoise / bdpt_last_preview_ms."""
    import pytest
    EINVAL, ESTATE = g._lib.BDPT_EINVAL, g._lib.BDPT_ESTATE
    W, H = 20, 19
    cam, sp = scene("cornell", W, H)
    with g.Renderer(sp, W, H, device=device) as r:
        with pytest.raises(g.BdptError) as e:                   # no camera yet
            r.preview_denoise()
        assert e.value.code == ESTATE
        with pytest.raises(g.BdptError) as e:
            r.last_preview_ms()
        assert e.value.code == ESTATE
        r.set_camera(cam)
        nan = float("nan")
        for bad in (dict(levels=-1), dict(levels=9), dict(normal_power=-1), dict(normal_power=7),
                    dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=nan), dict(sigma_color=-INF),
                    dict(count_ref=0.0), dict(count_ref=-1.0), dict(count_ref=nan), dict(count_ref=INF),
                    dict(count_ref=-INF), dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=nan),
                    dict(max_history=-INF), dict(plane_tol=-1e-3), dict(plane_tol=nan), dict(plane_tol=-INF)):
            with pytest.raises(g.BdptError) as e:
                r.preview_denoise(**bad)
            assert e.value.code == EINVAL, bad
        with pytest.raises(g.BdptError) as e:
            r.last_preview_ms()
        assert e.value.code == ESTATE                            # the failed calls do not count
        col = np.empty((H, W, 3), F)
        ptr = ctypes.c_void_p(col.ctypes.data)
        P = g._lib.PreviewParams
        prm = P(g._lib.ReprojectParams(0, 64.0, 0.01), 4, 5, 0.5, 8.0)
        assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(prm), None, None, None) == EINVAL   # all outputs NULL
        assert g.lib.bdpt_preview_denoise(r._h, None, ptr, None, None) == EINVAL                 # no parameters
        assert g.lib.bdpt_preview_denoise(None, ctypes.byref(prm), ptr, None, None) == EINVAL
        for m in (2, -1):
            bad = P(g._lib.ReprojectParams(m, 64.0, 0.01), 4, 5, 0.5, 8.0)
            assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(bad), ptr, None, None) == EINVAL
        with pytest.raises(g.BdptError) as e:
            r.last_preview_ms()
        assert e.value.code == ESTATE
        # valid at the ends of every range; a frame that was never rendered is all zeros and stays so
        out, w, px = r.preview_denoise(levels=8, normal_power=6, sigma_color=INF, count_ref=1e-30, max_history=INF,
                                       plane_tol=INF, materials="all", weight=True, pixels=True)
        assert out.shape == (H, W, 3) and w.shape == (H, W) and px.shape == (H, W, 4)
        assert (bits(out) == 0).all() and (bits(w) == 0).all() and not px.any()
        assert r.last_preview_ms() >= 0.0
        assert (bits(r.preview_denoise(levels=0, normal_power=0, sigma_color=1e-10, count_ref=3e38)) == 0).all()
        # each output alone through the C ABI
        wbuf, pbuf = np.ones((H, W), F), np.ones((H, W, 4), np.uint8)
        assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(prm), None, ctypes.c_void_p(wbuf.ctypes.data), None) == 0
        assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(prm), None, None, ctypes.c_void_p(pbuf.ctypes.data)) == 0
        assert (bits(wbuf) == 0).all() and not pbuf.any()


def assert_non_interference(device, name, W, H, streams=None):
    """4 passes + preview_denoise (defaults, and 8 levels with pixels) + 4 passes == 8 passes; on the
    GPU the call is queued behind unsynchronised passes, it saw the finished 4-pass frame, and the
    history read back before and after it is identical."""
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(8)
    col4, cnt4 = rendered(device, sp, W, H, cam, 4)
    hm = (cnt4.astype(F) * F(3)).astype(F)
    got, mid = [], []
    for probe in (False, True):
        with g.Renderer(sp, W, H, cam, device=device) as r:
            if streams is not None:
                r.set_streams(streams)
            r.light_pass(0)
            if probe:
                r.history_write(cam, col4, hm)
                before = r.history_read()
            r.path_passes(sid[:4], vlp[:4], sync=not probe)
            if probe:
                mid.append(r.preview_denoise(weight=True))
                r.preview_denoise(levels=8, materials="all", weight=True, pixels=True)
                after = r.history_read()
                same(after[0], before[0], "history colours before and after the call")
                same(after[1], before[1], "history weight before and after the call")
                assert r.history_info()[0] is True
            r.path_passes(sid[4:], vlp[4:])
            col, cnt = r.read_radiance()
            got.append((col, cnt, r.read_pixels(), r.read_rand(), r.read_lightpaths()))
    for a, b, what in zip(got[0], got[1], ("colors", "counter", "pixels", "rand", "lightpaths")):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what
    assert (got[0][1] == 8).all()
    aov = first_hit(sp, W, H, cam, device)
    o, a, _ = np_preview_denoise(col4, cnt4, aov, sp["refl"], hist_dict(cam, col4, hm, aov))
    same(mid[0][0], o, "the denoised preview of the 4-pass frame, queued behind unsynchronised passes, vs numpy")
    same(mid[0][1], a, "its count vs numpy")
