"""Shared by tests/test_denoise_cpu.py and tests/test_gpu_denoise.py (not a test module): the numpy
float32 statement of the denoiser's definition (include/bdpt.h bdpt_denoise),
vectorised over the pixels with a loop over the 25 taps, the frames and parameter sweep the tests
filter, and the checks both backends share.  Every comparison is on the bits of the float32
values; there is no tolerance."""
import itertools

import numpy as np

import gpu_bidirectional_raytracer_amd as g
from aov_common import bits, same, scene, schedule

F = np.float32
H5 = (F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16))
DEFAULTS = dict(levels=4, normal_power=5, sigma_color=0.5, materials="diffuse")
# levels 1, 3, 5 x both materials x normal_power 0, 5 x sigma_color 0.5, inf
SWEEP = [dict(levels=l, materials=m, normal_power=n, sigma_color=s)
         for l, m, n, s in itertools.product((1, 3, 5), ("diffuse", "all"), (0, 5), (0.5, float("inf")))]
# (scene, W, H): DIFF + REFR walls and ball + LITE emitter; misses; 783 spheres; a frame smaller than
# the later levels' steps (7x5: from step 8 on every off-centre tap is outside); DIFF + SPEC + REFR + LITE
FRAMES = [("cornell_glass", 65, 49), ("caustic", 40, 33), ("complex", 40, 33), ("cornell", 7, 5),
          ("cornell", 33, 25)]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def np_denoise(colors, ids, normals, refl, levels=4, normal_power=5, sigma_color=0.5, materials="diffuse"):
    """The definition, in float32 and in its operation order.  colors [H, W, 3], ids [H, W] (the
    unjittered first hit, -1 = miss), normals [H, W, 3], refl [n_spheres]."""
    cur = np.ascontiguousarray(colors, F).copy()
    ids = np.asarray(ids)
    normals = np.ascontiguousarray(normals, F)
    Hh, Ww = ids.shape
    elig = ids >= 0
    if materials == "diffuse":
        elig &= np.asarray(refl)[np.where(ids >= 0, ids, 0)] == g.DIFF
    with np.errstate(all="ignore"):
        isc0 = F(1.0) / (F(sigma_color) * F(sigma_color))
        for k in range(levels):
            s = 1 << k
            isc = isc0 * F(4 ** k)
            sw = np.zeros((Hh, Ww), F)
            sc = np.zeros((Hh, Ww, 3), F)
            for j in range(5):
                for i in range(5):
                    dy, dx = (j - 2) * s, (i - 2) * s
                    # centre rows / columns whose tap (y + dy, x + dx) is inside the frame
                    y0, y1 = max(0, -dy), min(Hh, Hh - dy)
                    x0, x1 = max(0, -dx), min(Ww, Ww - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    used = elig[P] & (ids[Q] == ids[P])
                    d = _dot(normals[P], normals[Q])
                    wn = np.where(d > 0, d, F(0))
                    for _ in range(normal_power):
                        wn = wn * wn
                    dc = cur[Q] - cur[P]
                    e2 = _dot(dc, dc)
                    wc = F(1) / (F(1) + e2 * isc)
                    w = ((H5[j] * H5[i]) * wn) * wc
                    assert w.dtype == F
                    sw[P] = np.where(used, sw[P] + w, sw[P])
                    sc[P] = np.where(used[..., None], sc[P] + w[..., None] * cur[Q], sc[P])
            r = F(1) / sw
            out = sc * r[..., None]
            assert out.dtype == F
            cur = np.where(elig[..., None], out, cur)
    return cur


def eligible(ids, refl, materials):
    e = ids >= 0
    if materials == "diffuse":
        e = e & (np.asarray(refl)[np.where(ids >= 0, ids, 0)] == g.DIFF)
    return e


def rendered_frame(device, name, W, H, npass=4):
    """(camera, spheres, colors, counter) after `npass` passes of the reference's schedule."""
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(npass)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        col, cnt = r.read_radiance()
    return cam, sp, col, cnt


def synthetic_radiance(W, H, seed=5):
    """Seeded finite values in [-1, 2) with 0, -0, 1e-30 and 1e18 sprinkled in and blocks of equal
    neighbours (dc = 0 exactly)."""
    rng = np.random.default_rng(seed)
    col = (rng.random((H, W, 3), dtype=F) * F(3) - F(1)).astype(F)
    special = np.array([0.0, -0.0, 1e-30, 1e18], F)
    pick = rng.integers(0, 12, (H, W, 3))
    col = np.where(pick < 4, special[np.minimum(pick, 3)], col).astype(F)
    for y, x in ((2, 3), (H // 2, W // 2), (H - 6, W - 7)):
        col[y:y + 5, x:x + 6] = col[y, x]
    col[0:3, 0:4] = F(1e-30)
    assert np.isfinite(col).all()
    return col


def to_rgba(col):
    """The toInt thresholds (bdpt_gamma_thresholds) and alpha 0 of bdpt_read_pixels."""
    import ctypes
    thr = np.zeros(256, F)
    g.lib.bdpt_gamma_thresholds(ctypes.c_void_p(thr.ctypes.data))
    k = np.searchsorted(thr, col, side="right") - 1
    k = np.where(np.isnan(col), 0, k)                     # every `v >= thr` fails for a NaN
    return np.concatenate([k.astype(np.uint8), np.zeros(col.shape[:2] + (1,), np.uint8)], axis=-1)


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_denoise / bdpt_last_denoise_ms."""
    import ctypes
    import pytest
    EINVAL, ESTATE = g._lib.BDPT_EINVAL, g._lib.BDPT_ESTATE
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, device=device) as r:
        with pytest.raises(g.BdptError) as e:               # no camera yet
            r.denoise()
        assert e.value.code == ESTATE
        with pytest.raises(g.BdptError) as e:               # and nothing denoised yet
            r.last_denoise_ms()
        assert e.value.code == ESTATE
        r.set_camera(cam)
        for bad in (dict(levels=0), dict(levels=9), dict(levels=-1), dict(normal_power=-1), dict(normal_power=7),
                    dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=float("nan")),
                    dict(sigma_color=float("-inf"))):
            with pytest.raises(g.BdptError) as e:
                r.denoise(**bad)
            assert e.value.code == EINVAL, bad
        with pytest.raises(g.BdptError) as e:
            r.last_denoise_ms()
        assert e.value.code == ESTATE                        # the failed calls do not count
        col = np.empty((19, 20, 3), F)
        ptr = ctypes.c_void_p(col.ctypes.data)
        prm = g._lib.DenoiseParams(4, 5, 0.5, 0)
        assert g.lib.bdpt_denoise(r._h, ctypes.byref(prm), None, None) == EINVAL     # both outputs NULL
        assert g.lib.bdpt_denoise(r._h, None, ptr, None) == EINVAL                   # no parameters
        for m in (2, -1):
            assert g.lib.bdpt_denoise(r._h, ctypes.byref(g._lib.DenoiseParams(4, 5, 0.5, m)), ptr, None) == EINVAL
        assert g.lib.bdpt_denoise(None, ctypes.byref(prm), ptr, None) == EINVAL
        # valid at the ends of every range; a frame that was never rendered is all zeros and stays so
        assert (bits(r.denoise(levels=1, normal_power=0, sigma_color=1e-10)) == 0).all()
        out, px = r.denoise(levels=8, normal_power=6, sigma_color=float("inf"), materials="all", pixels=True)
        assert out.shape == (19, 20, 3) and px.shape == (19, 20, 4) and (bits(out) == 0).all() and not px.any()
        assert r.last_denoise_ms() >= 0.0


def assert_non_interference(device, name, W, H, streams=None):
    """4 passes, denoise (defaults and an 8-level one with pixels), 4 passes == 8 passes; on the
    GPU the denoise is queued behind unsynchronised passes."""
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(8)
    got, mid = [], []
    for probe in (False, True):
        with g.Renderer(sp, W, H, cam, device=device) as r:
            if streams is not None:
                r.set_streams(streams)
            r.light_pass(0)
            r.path_passes(sid[:4], vlp[:4], sync=not probe)
            if probe:
                mid.append(r.denoise())
                r.denoise(levels=8, materials="all", pixels=True)
            r.path_passes(sid[4:], vlp[4:])
            col, cnt = r.read_radiance()
            got.append((col, cnt, r.read_pixels(), r.read_rand(), r.read_lightpaths()))
    for a, b, what in zip(got[0], got[1], ("colors", "counter", "pixels", "rand", "lightpaths")):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what
    assert (got[0][1] == 8).all()
    # and the frame it filtered was the finished 4-pass frame, though nothing had waited for it
    with g.Renderer(sp, W, H, cam, device=device) as r:
        if streams is not None:
            r.set_streams(streams)
        r.light_pass(0)
        r.path_passes(sid[:4], vlp[:4])
        col4, _ = r.read_radiance()
        same(r.denoise(), mid[0], "the denoised 4-pass frame, queued behind unsynchronised passes or not")
        aov = r.render_aov()
    same(np_denoise(col4, aov["id"], aov["normal"], sp["refl"]), mid[0], "the denoised 4-pass frame vs numpy")
