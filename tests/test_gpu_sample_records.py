"""Sample records on the GPU (bdpt_kernels.hip BDPT_SREC, bdpt_sample_records_kernel): the
specialised pass-stream kernels load, per path segment, one 32-B record of everything the segment
takes from d_Rand[j..j+4] instead of computing it per vertex.

 (a) the table read back (bdpt_read_sample_records) equals the NumPy restatement
     (tests/sample_records_ref.py) on every position, for two seeds;
 (b) frames are the oracle's bit for bit -- packed-edge sizes, 16 passes, three scenes, sids at the
     table's wrap (RAND_N - 6, RAND_N - 31) and in every residue class mod 25 (the planes) -- in
     the auto mode, with one pass per lane, and with the ordered in-kernel fold, each with records
     and with BDPT_JIT_FLAGS=-DBDPT_SREC=0 (the sin/cos planes);
 (c) the derived tables are rebuilt after every table change before a kernel reads them
     (light pass, bdpt_generate_rand, specialisation off and on again);
 (d) a two-shard context on one GPU (each shard owns its tables) equals the single context;
 (e) a retired switch in BDPT_JIT_FLAGS fails the specialised build, and the call falls back to the
     precompiled instance with the same frame."""
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
import oracle
from conftest import SCENES
from sample_records_ref import records

pytestmark = pytest.mark.gpu
RAND_N = g.RAND_N
M5 = RAND_N - 5


@pytest.fixture(scope="module")
def tables():
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = oracle.mt607(seed)
        return cache[seed]
    return get


def _scene(name, W, H):
    cam, sp = g.read_scene(os.path.join(SCENES, name + ".scn"))
    g.update_camera(cam, W, H)
    return cam, sp


def _same(got, want, what):
    col, cnt, px = got
    ocol, ocnt, opx = want
    assert np.array_equal(cnt, ocnt), what
    assert np.array_equal(col.view(np.uint32), ocol.view(np.uint32)), \
        f"{what}: {int((col != ocol).sum())} values differ"
    assert np.array_equal(px, opx), what


def test_records_equal_restatement(gpu, tables):
    cam, sp = _scene("simple", 17, 9)
    pos = np.arange(M5)
    with g.Renderer(sp, 17, 9, cam, device=gpu) as r:
        for seed in (0, 5):
            r.generate_rand(seed)
            table = r.read_rand()
            assert np.array_equal(table, tables(seed))
            got = r.read_sample_records()
            assert got.shape == (M5, 8)
            want = records(table, pos)
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
            assert bad.size == 0, (seed, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _sids(which):
    """16 sids: the two at the table's wrap and one per residue class mod 25 -- classes 0..13 in
    set 0, 11..24 in set 1 (16 passes hold 14 classes; the two frame sizes take one set each)."""
    rng = np.random.default_rng(25 + which)
    classes = range(0, 14) if which == 0 else range(11, 25)
    res = [int(rng.integers(0, RAND_N // 25 - 1)) * 25 + c for c in classes]
    return np.array([RAND_N - 6, RAND_N - 31] + res, np.uint32)


MODES = [("auto", 0, None), ("lane", -1, None), ("units", -1, "8")]


@pytest.mark.parametrize("which,W,H", [(0, 33, 25), (1, 65, 17)])
@pytest.mark.parametrize("name", ["cornell", "cornell_glass", "cornell_2luci"])
def test_frames_match_oracle(gpu, tables, name, which, W, H, monkeypatch):
    sid = _sids(which)
    assert len(sid) == 16 and {int(s) % 25 for s in sid} >= set(range(0, 14) if which == 0 else range(11, 25))
    s = g.PassScheduler()
    s.light()
    _, vlp = s.next(16)
    cam, sp = _scene(name, W, H)
    rnd0 = tables(0)
    want = oracle.path_passes(sp, rnd0, cam, W, H, oracle.light_pass(sp, rnd0, 0), sid, vlp)
    for mode, streams, units in MODES:
        for srec in (True, False):
            if units:
                monkeypatch.setenv("BDPT_UNITS", units)
            else:
                monkeypatch.delenv("BDPT_UNITS", raising=False)
            if srec:
                monkeypatch.delenv("BDPT_JIT_FLAGS", raising=False)
            else:
                monkeypatch.setenv("BDPT_JIT_FLAGS", "-DBDPT_SREC=0")
            what = f"{name} {W}x{H} {mode} records={srec}"
            with g.Renderer(sp, W, H, cam, device=gpu) as r:
                r.set_streams(streams)
                r.light_pass(0)
                r.path_passes(sid, vlp)
                feats = r.last_features
                assert r.last_streams > 1 and r.last_specialized, (what, r.specialize_status)
                assert ("unit_fold" in feats) == bool(units), (what, feats)
                assert ("sample_records" in feats) == srec and "sincos_planes" in feats, (what, feats)
                col, cnt = r.read_radiance()
                _same((col, cnt, r.read_pixels()), want, what)


def test_tables_follow_the_random_table(gpu, tables):
    """Every step changes the table or the kernel that reads a derived table; the frame must be
    the oracle's for the table then in force (VLPs: the light pass of sample 0 throughout)."""
    W, H = 33, 25
    cam, sp = _scene("cornell", W, H)
    s = g.PassScheduler()
    s.light()
    sid, vlp = s.next(4)
    lp = oracle.light_pass(sp, tables(0), 0)

    def check(r, seed, specialised, what):
        r.reset_accum()
        r.path_passes(sid, vlp)
        feats = r.last_features
        assert r.last_specialized == specialised and ("sample_records" in feats) == specialised, (what, feats)
        assert "sincos_planes" in feats, (what, feats)
        col, cnt = r.read_radiance()
        want = oracle.path_passes(sp, tables(seed), cam, W, H, lp, sid, vlp)
        _same((col, cnt, r.read_pixels()), want, what)

    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.set_streams(-1)
        r.light_pass(0)
        check(r, 0, True, "light_pass(0)")
        r.generate_rand(5)
        check(r, 5, True, "generate_rand(5)")
        r.set_specialize(False)
        check(r, 5, False, "set_specialize(False)")       # the planes' first use
        r.set_specialize(True)
        check(r, 5, True, "set_specialize(True)")
        # both derived tables exist now and are stale after the next table
        r.generate_rand(7)
        check(r, 7, True, "generate_rand(7)")
        r.set_specialize(False)
        check(r, 7, False, "generate_rand(7), planes")


def test_retired_switch_falls_back_to_the_precompiled_kernel(gpu, tables, monkeypatch):
    """A retired switch in BDPT_JIT_FLAGS fails the specialised build (the guard at the top of
    bdpt_kernels.hip) instead of building the default kernel under another name: the call runs
    the precompiled instance, says why, and the frame is still the oracle's."""
    W, H = 33, 25
    cam, sp = _scene("cornell", W, H)
    s = g.PassScheduler()
    s.light()
    sid, vlp = s.next(4)
    rnd0 = tables(0)
    want = oracle.path_passes(sp, rnd0, cam, W, H, oracle.light_pass(sp, rnd0, 0), sid, vlp)
    for flags, specialised in (("-DBDPT_LG_RULE=0", False), (None, True)):
        if flags:
            monkeypatch.setenv("BDPT_JIT_FLAGS", flags)
        else:
            monkeypatch.delenv("BDPT_JIT_FLAGS", raising=False)
        with g.Renderer(sp, W, H, cam, device=gpu) as r:
            r.set_streams(-1)
            r.light_pass(0)
            r.path_passes(sid, vlp)
            assert r.last_specialized == specialised, (flags, r.specialize_status)
            if not specialised:
                assert "BDPT_LG_RULE" in r.specialize_status, r.specialize_status
            col, cnt = r.read_radiance()
            _same((col, cnt, r.read_pixels()), want, f"BDPT_JIT_FLAGS={flags}")


def test_two_shards_equal_single_context(gpu, tables):
    W, H = 33, 25
    cam, sp = _scene("cornell", W, H)
    s = g.PassScheduler()
    s.light()
    sid, vlp = s.next(16)
    frames = []
    for kw in (dict(device=gpu), dict(devices=[gpu, gpu])):
        with g.Renderer(sp, W, H, cam, **kw) as r:
            r.set_streams(-1)
            r.light_pass(0)
            r.path_passes(sid, vlp)
            for k in range(r.num_devices):
                assert "sample_records" in r.device_mode(k)["features"], (kw, k, r.device_mode(k))
            col, cnt = r.read_radiance()
            frames.append((col, cnt, r.read_pixels()))
    _same(frames[1], frames[0], "devices=[0, 0]")
    rnd0 = tables(0)
    _same(frames[0], oracle.path_passes(sp, rnd0, cam, W, H, oracle.light_pass(sp, rnd0, 0), sid, vlp), "single")
