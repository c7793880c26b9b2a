"""Shared by tests/test_aov_cpu.py and tests/test_gpu_aov.py (not a test module): rendering the
first-hit feature buffers of a fixture or a scene, and what the reference's colours say about them.
Every comparison is on the bits of the float32 values; there is no tolerance."""
import json
import os

import numpy as np

import gpu_bidirectional_raytracer_amd as g
from conftest import GOLDEN, SCENES
from make_ref_aov_golden import load_case, probe_scene

AOV_META = json.load(open(os.path.join(GOLDEN, "ref_aov_meta.json")))
CASES = [c["name"] for c in AOV_META["cases"]]
PLANES = g.AOV_PLANES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bad = int((bits(a) != bits(b)).sum())
    assert bad == 0, f"{what}: {bad} of {a.size} values differ"


def same_aov(a, b, what):
    assert sorted(a) == sorted(b) == sorted(PLANES)
    for k in PLANES:
        same(a[k], b[k], f"{what}: {k}")


def camera_of(fx):
    return g.Camera.from_buffer_copy(np.ascontiguousarray(fx["camera"]).tobytes())


def render_fixture(fx, device, traversal=None):
    """render_aov of a ref_aov_* fixture's inputs -> (planes, last_aov_traversal)."""
    with g.Renderer(fx["spheres"], fx["W"], fx["H"], camera_of(fx), device=device) as r:
        if traversal is not None:
            r.set_traversal(traversal)
        if fx["table_seed"] >= 0:
            r.generate_rand(fx["table_seed"])
            aov = r.render_aov(sid=fx["sid"])
        else:
            aov = r.render_aov()                    # the zero table: no jitter, no table at all
        return aov, r.last_aov_traversal


def probe_colors(spheres, aov):
    """e[id] * |dp| per channel in float32 (device.cu:651-660 with throughput 1), +0 on a miss."""
    hit = aov["id"] >= 0
    e = np.ascontiguousarray(spheres["e"], np.float32)[np.where(hit, aov["id"], 0)]
    col = e * np.abs(aov["dp"])[..., None]
    assert col.dtype == np.float32
    col[~hit] = 0.0
    return col


def assert_matches_reference(fx, aov, what):
    col = fx["colors"]
    same(probe_colors(fx["spheres"], aov), col, f"{what}: e[id] * |dp| vs the reference's colours")
    miss = aov["id"] == -1
    assert np.array_equal(miss, (bits(col) == 0).all(axis=-1)), f"{what}: misses are not the all-zero pixels"
    assert ((aov["id"] >= -1) & (aov["id"] < len(fx["spheres"]))).all()


def scene(name, W, H, probe=False):
    cam, sp = g.read_scene(os.path.join(SCENES, name + ".scn"))
    g.update_camera(cam, W, H)
    return cam, (probe_scene(sp) if probe else sp)


def schedule(n):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


def assert_window_slices(r, whole, sid, windows, what):
    """Windows (and pick for the 1x1 ones) equal the slices of the whole frame."""
    for x0, y0, w, h in windows:
        win = r.render_aov(sid=sid, window=(x0, y0, w, h))
        for k in PLANES:
            same(win[k], whole[k][y0:y0 + h, x0:x0 + w], f"{what}: window {(x0, y0, w, h)} {k}")
        if (w, h) == (1, 1):
            i, t = r.pick(x0, y0, sid=sid)
            assert i == int(whole["id"][y0, x0])
            assert np.float32(t).view(np.uint32) == bits(whole["t"])[y0, x0]


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_render_aov."""
    import pytest
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, device=device) as r:
        with pytest.raises(g.BdptError) as e:                       # no camera yet
            r.render_aov()
        assert e.value.code == g._lib.BDPT_ESTATE
        with pytest.raises(g.BdptError) as e:
            r.pick(0, 0)
        assert e.value.code == g._lib.BDPT_ESTATE
        with pytest.raises(g.BdptError) as e:
            _ = r.last_aov_traversal
        assert e.value.code == g._lib.BDPT_ESTATE
        r.set_camera(cam)
        assert r.render_aov()["id"].shape == (19, 20)               # no jitter needs no table
        with pytest.raises(g.BdptError) as e:                       # jitter before a table exists
            r.render_aov(sid=7)
        assert e.value.code == g._lib.BDPT_ESTATE
        with pytest.raises(g.BdptError) as e:
            r.pick(3, 3, sid=7)
        assert e.value.code == g._lib.BDPT_ESTATE
        r.generate_rand(15)
        r.render_aov(sid=g.RAND_N - 1)
        for bad in ((0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (-1, 0, 5, 5), (0, -1, 5, 5), (16, 0, 5, 5),
                    (0, 15, 5, 5), (20, 0, 1, 1), (0, 19, 1, 1), (0, 0, 21, 19), (0, 0, 20, 20),
                    (2 ** 31 - 1, 0, 2, 1)):
            with pytest.raises(g.BdptError) as e:
                r.render_aov(window=bad)
            assert e.value.code == g._lib.BDPT_EINVAL, bad
        for x, y in ((20, 0), (0, 19), (-1, 0)):
            with pytest.raises(g.BdptError) as e:
                r.pick(x, y)
            assert e.value.code == g._lib.BDPT_EINVAL
        with pytest.raises(g.BdptError) as e:
            r.render_aov(sid=g.RAND_N)
        assert e.value.code == g._lib.BDPT_EINVAL
        with pytest.raises(g.BdptError) as e:
            r.pick(0, 0, sid=g.RAND_N)
        assert e.value.code == g._lib.BDPT_EINVAL
        assert g.lib.bdpt_render_aov(r._h, 0, 0, 1, 1, 0, 0, None) == g._lib.BDPT_EINVAL   # NULL `out`
        assert r.render_aov(window=(19, 18, 1, 1))["id"].shape == (1, 1)   # the last pixel is inside


def assert_non_interference(device, name, W, H, streams=None):
    """4 passes, render_aov (whole frame, a window, a pick; jittered and not), 4 passes == 8 passes."""
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(8)
    got = []
    for probe in (False, True):
        with g.Renderer(sp, W, H, cam, device=device) as r:
            if streams is not None:
                r.set_streams(streams)
            r.light_pass(0)
            r.path_passes(sid[:4], vlp[:4], sync=not probe)
            if probe:
                r.render_aov(sid=int(sid[0]))
                r.render_aov(window=(3, 2, 9, 5))
                r.pick(W // 2, H // 2, sid=int(sid[1]))
            r.path_passes(sid[4:], vlp[4:])
            col, cnt = r.read_radiance()
            got.append((col, cnt, r.read_pixels(), r.read_rand(), r.read_lightpaths()))
    for a, b, what in zip(got[0], got[1], ("colors", "counter", "pixels", "rand", "lightpaths")):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what
    assert (got[0][1] == 8).all()


CLOCKS = ("aov", "denoise", "reproject", "preview", "noise")     # the bdpt_last_*_ms readers, by service


def assert_only_own_clock_answers(device, service):
    """A fresh context with a camera, a light pass and one path pass: no last_*_ms answers before a
    service has run (BDPT_ESTATE); after `service` alone only its own reader does, >= 0 on the CPU
    backend and > 0 on a GPU.  denoise / reproject / preview_denoise run the first-hit kernel
    themselves but are not render_aov, so last_aov_ms stays unanswered after them."""
    import pytest
    cam, sp = scene("cornell", 20, 19)
    sid, vlp = schedule(2)
    calls = {"aov": lambda r: r.render_aov(), "denoise": lambda r: r.denoise(levels=2),
             "reproject": lambda r: r.reproject(), "preview": lambda r: r.preview_denoise(levels=2),
             "noise": lambda r: r.noise_estimate()}
    assert set(calls) == set(CLOCKS)

    def answering(r):
        out = {}
        for k in CLOCKS:
            try:
                out[k] = getattr(r, f"last_{k}_ms")()
            except g.BdptError as e:
                assert e.code == g._lib.BDPT_ESTATE, (k, e)
        return out

    with g.Renderer(sp, 20, 19, cam, device=device) as r:
        r.light_pass(0)
        r.path_passes(sid[:1], vlp[:1])
        if service == "noise":                                          # an estimate measures against a mark
            r.noise_mark()
            r.path_passes(sid[1:], vlp[1:])
        assert answering(r) == {}, "a reader answered before any service ran"
        calls[service](r)
        ms = answering(r)
        assert list(ms) == [service], f"after {service} alone: {sorted(ms)} answer"
        assert ms[service] >= 0.0 if device < 0 else ms[service] > 0.0, ms
