"""Shared by tests/test_reproject_cpu.py and tests/test_gpu_reproject.py (not a test module): the
numpy float32 statement of the temporal reprojection (include/bdpt.h bdpt_reproject),
vectorised over the pixels with a loop over the four taps, the camera constants restated in numpy,
the frames, camera moves and parameter sweep the tests use, and the checks both backends share.
Every comparison of a backend with the statement or with the other backend is on the bits of the
float32 values; there is no tolerance."""
import ctypes
import functools
import itertools

import numpy as np

import gpu_bidirectional_raytracer_amd as g
from aov_common import bits, same, scene, schedule
from denoise_common import eligible, synthetic_radiance, to_rgba

F = np.float32
INF = float("inf")
CPU = -1
DEFAULTS = dict(max_history=64.0, plane_tol=0.01, materials="diffuse")
# both materials x max_history 1, 64, inf x plane_tol 0, 0.01, inf
SWEEP = [dict(materials=m, max_history=h, plane_tol=t)
         for m, h, t in itertools.product(("diffuse", "all"), (1.0, 64.0, INF), (0.0, 0.01, INF))]
# (scene, W, H, traversal of the first hits): none a multiple of the 8x8 / 64x1 wave tiles or of the
# 32x8 / 64x4 workgroup tiles; caustic has misses, complex 783 spheres and a BVH
FRAMES = [("cornell", 65, 49, None), ("cornell_glass", 40, 33, None), ("caustic", 40, 33, None),
          ("complex", 40, 33, "brute"), ("complex", 40, 33, "bvh"), ("cornell", 7, 5, None), ("cornell", 129, 3, None)]
# camera keys between the history's view and the current one; after the last, much of the frame
# falls outside the old view
KEYSETS = [(" ",), ("a",), ("left",), ("w", "up"), ("a", "a", "a", "left", "left", "left", "left")]
MOVES = KEYSETS[1:]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _vec(v):
    return np.array([v.x, v.y, v.z], F)


def _vnorm3(v):
    l = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    assert l.dtype == F
    return np.array([l * v[0], l * v[1], l * v[2]], F)


def camera_constants(cam, W, H):
    """ux, uy, ud, o, hw, hh, sx, sy of the history's camera, as camera_args forms them."""
    inv_w, inv_h = F(14.0 / W), F(10.5 / H)
    hw = F(float(inv_w * F(W)) / 2.0)
    hh = F(float(inv_h * F(H)) / 2.0)
    return (_vnorm3(_vec(cam.x)), _vnorm3(_vec(cam.y)), _vnorm3(_vec(cam.dir)), _vec(cam.orig), hw, hh,
            F(1) / inv_w, F(1) / inv_h)


def np_reproject(colors, counter, aov, refl, hist, max_history=64.0, plane_tol=0.01, materials="diffuse"):
    """The definition, in float32 and in its operation order.  colors [H, W, 3] and counter [H, W] as
    read_radiance returns them, aov: the current camera's unjittered first hit (id, t, position,
    normal), refl [n_spheres], hist: None or dict(camera, hc, hm, gid, gpos).  Returns (out, weight,
    taps used per pixel)."""
    col = np.ascontiguousarray(colors, F)
    n = np.asarray(counter).astype(F)
    Hh, Ww = n.shape
    id1, t1 = np.asarray(aov["id"]), np.ascontiguousarray(aov["t"], F)
    P, N = np.ascontiguousarray(aov["position"], F), np.ascontiguousarray(aov["normal"], F)
    m = np.zeros((Hh, Ww), F)
    h = np.zeros((Hh, Ww, 3), F)
    taps = np.zeros((Hh, Ww), np.int32)
    with np.errstate(all="ignore"):
        if hist is not None:
            ux, uy, ud, o, hw, hh, sx, sy = camera_constants(hist["camera"], Ww, Hh)
            gid, hm = np.asarray(hist["gid"]), np.ascontiguousarray(hist["hm"], F)
            gpos, hc = np.ascontiguousarray(hist["gpos"], F), np.ascontiguousarray(hist["hc"], F)
            v = P - o
            a, b, cz = _dot(v, ux), _dot(v, uy), _dot(v, ud)
            r = F(1) / cz
            kx, ky = (F(10) * a) * r, (F(10) * b) * r
            fx, fy = (kx + hw) * sx, (ky + hh) * sy
            assert fx.dtype == F and fy.dtype == F
            ok = eligible(id1, refl, materials) & (fx >= F(-1)) & (fx < F(Ww)) & (fy >= F(-1)) & (fy < F(Hh))
            xf, yf = np.floor(fx), np.floor(fy)
            wx, wy = fx - xf, fy - yf
            x0 = np.where(ok, xf, F(0)).astype(np.int64)
            y0 = np.where(ok, yf, F(0)).astype(np.int64)
            lim = F(plane_tol) * t1
            sw, sm, sc = np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F), np.zeros((Hh, Ww, 3), F)
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = x0 + dx, y0 + dy
                    bx = wx if dx else F(1) - wx
                    by = wy if dy else F(1) - wy
                    bw = bx * by
                    inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                    Q = (np.clip(qy, 0, Hh - 1), np.clip(qx, 0, Ww - 1))
                    hmq = hm[Q]
                    use = ok & inside & (bw > 0) & (gid[Q] == id1) & (hmq > 0)
                    use &= np.abs(_dot(gpos[Q] - P, N)) <= lim
                    sw = np.where(use, sw + bw, sw)
                    sm = np.where(use, sm + bw * np.minimum(hmq, F(max_history)), sm)
                    sc = np.where(use[..., None], sc + bw[..., None] * hc[Q], sc)
                    taps += use
            assert sw.dtype == F and sm.dtype == F and sc.dtype == F
            h = sc * (F(1) / sw)[..., None]
            m = np.where(taps > 0, sm, F(0))
        tot = n + m
        blend = (n[..., None] * col + m[..., None] * h) * (F(1) / tot)[..., None]
        assert blend.dtype == F and tot.dtype == F
        out = np.where((m == 0)[..., None], col, np.where((n == 0)[..., None], h, blend))
    return out, tot, taps


def copy_camera(cam):
    return g.Camera.from_buffer_copy(bytes(cam))


def moved(cam, keys, W, H):
    """The camera after the keys, each followed by ReInit's UpdateCamera."""
    cam = copy_camera(cam)
    for k in keys:
        assert g.camera_key(cam, k)
        g.update_camera(cam, W, H)
    return cam


def first_hit(sp, W, H, cam, device=CPU, traversal=None):
    with g.Renderer(sp, W, H, cam, device=device) as r:
        if traversal:
            r.set_traversal(traversal)
        return r.render_aov()


def rendered(device, sp, W, H, cam, npass):
    sid, vlp = schedule(npass)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        return r.read_radiance()


def patterned_weight(W, H):
    """A different count from pixel to pixel, zeros and fractions included."""
    y, x = np.mgrid[0:H, 0:W]
    return (((x * 7 + y * 3) % 5).astype(F) * F(0.75)).astype(F)


@functools.lru_cache(maxsize=None)
def history_of(name, W, H):
    """(cam0, spheres, 4-pass colours under cam0, their float count, cam0's first hit), rendered on the
    CPU backend once per frame and never modified."""
    cam0, sp = scene(name, W, H)
    col, cnt = rendered(CPU, sp, W, H, cam0, 4)
    assert (cnt == 4).all() and np.isfinite(col).all()
    return cam0, sp, col, cnt.astype(F), first_hit(sp, W, H, cam0)


@functools.lru_cache(maxsize=None)
def case_of(name, W, H, keys):
    """history_of plus the view after `keys`: (cam1, 1-pass colours and counter under cam1, cam1's
    first hit)."""
    cam0, sp, _, _, _ = history_of(name, W, H)
    cam1 = moved(cam0, keys, W, H)
    col, cnt = rendered(CPU, sp, W, H, cam1, 1)
    return cam1, col, cnt, first_hit(sp, W, H, cam1)


def hist_dict(cam0, hc, hm, aov0):
    return dict(camera=cam0, hc=hc, hm=hm, gid=aov0["id"], gpos=aov0["position"])


def assert_sweep(device, name, W, H, traversal, keys, hm=None, params=SWEEP):
    """History written under the old camera, one pass under the new one: reproject and the capture's
    history_read equal the statement over the sweep.  Returns the statement's results."""
    cam0, sp, hc, hm4, aov0 = history_of(name, W, H)
    hm = hm4 if hm is None else hm
    cam1, col, cnt, aov1 = case_of(name, W, H, keys)
    hist = hist_dict(cam0, hc, hm, aov0)
    want = []
    with g.Renderer(sp, W, H, cam1, device=device) as r:
        if traversal:
            r.set_traversal(traversal)
        r.write_radiance(col, cnt)
        for prm in params:
            r.history_write(cam0, hc, hm)
            what = f"{name} {W}x{H} {traversal} {keys} {prm}"
            o, w, _ = np_reproject(col, cnt, aov1, sp["refl"], hist, **prm)
            got, gw = r.reproject(weight=True, **prm)
            same(got, o, what + ": out")
            same(gw, w, what + ": weight")
            r.history_capture(**prm)
            c2, w2 = r.history_read()
            same(c2, o, what + ": captured colours")
            same(w2, w, what + ": captured weight")
            want.append((o, w))
        same(r.read_radiance()[0], col, "the accumulation is only read")
    return want


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_reproject and the history entry points."""
    import pytest
    EINVAL, ESTATE = g._lib.BDPT_EINVAL, g._lib.BDPT_ESTATE
    W, H = 20, 19
    cam, sp = scene("cornell", W, H)
    with g.Renderer(sp, W, H, device=device) as r:
        for call in (r.reproject, r.history_capture):           # no camera yet
            with pytest.raises(g.BdptError) as e:
                call()
            assert e.value.code == ESTATE
        with pytest.raises(g.BdptError) as e:
            r.last_reproject_ms()
        assert e.value.code == ESTATE
        with pytest.raises(g.BdptError) as e:
            r.history_read()
        assert e.value.code == ESTATE
        assert r.history_info() == (False, None)
        r.set_camera(cam)
        for bad in (dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=float("nan")),
                    dict(max_history=-INF), dict(plane_tol=-1e-3), dict(plane_tol=float("nan")), dict(plane_tol=-INF)):
            for call in (r.reproject, r.history_capture):
                with pytest.raises(g.BdptError) as e:
                    call(**bad)
                assert e.value.code == EINVAL, bad
        with pytest.raises(g.BdptError) as e:
            r.last_reproject_ms()
        assert e.value.code == ESTATE                            # the failed calls do not count
        assert r.history_info() == (False, None)                 # nor did a failed capture store anything
        col = np.empty((H, W, 3), F)
        ptr = ctypes.c_void_p(col.ctypes.data)
        prm = g._lib.ReprojectParams(0, 64.0, 0.01)
        assert g.lib.bdpt_reproject(r._h, ctypes.byref(prm), None, None, None) == EINVAL   # all outputs NULL
        assert g.lib.bdpt_reproject(r._h, None, ptr, None, None) == EINVAL                 # no parameters
        assert g.lib.bdpt_history_capture(r._h, None) == EINVAL
        for m in (2, -1):
            bad = g._lib.ReprojectParams(m, 64.0, 0.01)
            assert g.lib.bdpt_reproject(r._h, ctypes.byref(bad), ptr, None, None) == EINVAL
            assert g.lib.bdpt_history_capture(r._h, ctypes.byref(bad)) == EINVAL
        assert g.lib.bdpt_reproject(None, ctypes.byref(prm), ptr, None, None) == EINVAL
        assert g.lib.bdpt_history_write(r._h, None, ptr, ptr) == EINVAL
        assert g.lib.bdpt_history_write(r._h, ctypes.byref(cam), None, ptr) == EINVAL
        assert g.lib.bdpt_history_write(r._h, ctypes.byref(cam), ptr, None) == EINVAL
        # without a history: the input, a frame never rendered being all zeros with count 0
        out, w, px = r.reproject(weight=True, pixels=True, max_history=INF, plane_tol=INF, materials="all")
        assert out.shape == (H, W, 3) and w.shape == (H, W) and px.shape == (H, W, 4)
        assert (bits(out) == 0).all() and (bits(w) == 0).all() and not px.any()
        assert r.last_reproject_ms() >= 0.0
        # each output alone through the C ABI
        wbuf, pbuf = np.empty((H, W), F), np.empty((H, W, 4), np.uint8)
        assert g.lib.bdpt_reproject(r._h, ctypes.byref(prm), None, ctypes.c_void_p(wbuf.ctypes.data), None) == 0
        assert g.lib.bdpt_reproject(r._h, ctypes.byref(prm), None, None, ctypes.c_void_p(pbuf.ctypes.data)) == 0
        assert (bits(wbuf) == 0).all() and not pbuf.any()
        r.history_capture()
        present, c0 = r.history_info()
        assert present and bytes(c0) == bytes(cam)
        r.history_clear()
        assert r.history_info()[0] is False
        with pytest.raises(g.BdptError) as e:
            r.history_read()
        assert e.value.code == ESTATE


def assert_non_interference(device, name, W, H, streams=None):
    """4 passes, capture + reproject (defaults and another parameter set with weight and pixels),
    4 passes == 8 passes; on the GPU they are queued behind unsynchronised passes, and what they saw
    was the finished 4-pass frame."""
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
                r.history_capture()
                mid.append(r.history_read())
                mid.append(r.reproject(weight=True))
                r.reproject(max_history=1.0, plane_tol=INF, materials="all", weight=True, pixels=True)
                r.history_capture(materials="all")
            r.path_passes(sid[4:], vlp[4:])
            col, cnt = r.read_radiance()
            got.append((col, cnt, r.read_pixels(), r.read_rand(), r.read_lightpaths()))
    for a, b, what in zip(got[0], got[1], ("colors", "counter", "pixels", "rand", "lightpaths")):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what
    assert (got[0][1] == 8).all()
    col4, cnt4 = rendered(device, sp, W, H, cam, 4)
    same(mid[0][0], col4, "the captured frame, queued behind unsynchronised passes")
    same(mid[0][1], cnt4.astype(F), "the captured weight")
    aov = first_hit(sp, W, H, cam, device)
    o, w, _ = np_reproject(col4, cnt4, aov, sp["refl"], hist_dict(cam, col4, cnt4.astype(F), aov))
    same(mid[1][0], o, "reprojection onto the same view vs numpy")
    same(mid[1][1], w, "its weight vs numpy")
