"""BASELINE.json configs at their full sizes (internal = CLI + 1), on one GPU, each compared with
the oracle on a real fraction of the frame (bit-exact; the north star's L-inf < 1e-3 is implied):

configs[1] cornell 513x513, 256 spp      -> whole frame; and the north star's tolerance check,
           L-inf < 1e-3 after 1024 spp, on the whole 513x513 frame
configs[2] cornell_glass 1921x1081, 1024 spp -> every 32nd row (34 rows, 3 % of the frame) + the
           last row; counters and pixel = toInt(colors) on the whole frame (and the whole frame
           at 128 spp vs the oracle in the kernel-mode test below)
configs[3] caustic 1921x1081, 4096 spp on 8 pixel-band shards -> shard sum == one-context
           frame bit for bit (the RCCL reduce is a sum of disjoint frames); the whole summed
           frame vs the oracle at the full 4096 spp (8.5 G oracle samples, about a minute)
configs[4] synthetic64 4097x4097 -> one 4097x512 band (what one of 8 GPUs renders) at the
           full 8192 spp (vlp_index wraps inside the run): ownership and counters over the frame;
           whole 8-row tile bands at the start, middle and end of the GPU's band vs the oracle
           (24 of 512 rows)
"""
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
import oracle
from conftest import SCENES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rnd0():
    return oracle.mt607(0)


def _setup(name, W, H, gpu):
    cam, sp = g.read_scene(os.path.join(SCENES, name + ".scn"))
    g.update_camera(cam, W, H)
    r = g.Renderer(sp, W, H, cam, device=gpu)
    r.light_pass(0)
    return r, cam, sp


def _schedule(n):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


def _same(a, b, what):
    if a.dtype.kind == "f":
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first at {bad[:3].tolist()}"


def _pixels_are_toint(r, col):
    thr = np.zeros(256, np.float32)
    g._lib.lib.bdpt_gamma_thresholds(g._lib.ctypes.c_void_p(thr.ctypes.data))
    k = np.searchsorted(thr, col.reshape(-1), side="right").reshape(col.shape) - 1
    _same(r.read_pixels()[..., :3], k.astype(np.uint8), "pixels vs toInt(colors)")


def test_config1_cornell_513_256spp_full_frame(gpu, rnd0):
    W, H, spp = 513, 513, 256
    r, cam, sp = _setup("cornell", W, H, gpu)
    sid, vlp = _schedule(spp)
    r.path_passes(sid, vlp)
    col, cnt = r.read_radiance()
    lp = oracle.light_pass(sp, rnd0, 0)
    ocol, ocnt, opix = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp)
    _same(cnt, ocnt, "counter")
    _same(col, ocol, "colors")
    _same(r.read_pixels(), opix, "pixels")
    r.close()


def test_config2_cornell_glass_1080p_1024spp(gpu, rnd0):
    W, H, spp = 1921, 1081, 1024
    r, cam, sp = _setup("cornell_glass", W, H, gpu)
    sid, vlp = _schedule(spp)
    r.path_passes(sid, vlp)
    col, cnt = r.read_radiance()
    assert (cnt == spp).all() and np.isfinite(col).all() and (col >= 0).all()
    _pixels_are_toint(r, col)
    lp = oracle.light_pass(sp, rnd0, 0)
    for y in list(range(0, H, 32)) + [H - 1]:
        ocol, ocnt, _ = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp, rows=(y, y + 1))
        _same(col[y], ocol[y], f"row {y}")
        _same(cnt[y], ocnt[y], f"row {y} counters")
    r.close()


def test_config3_caustic_1080p_4096spp_8_shards(gpu, rnd0):
    W, H, spp, N = 1921, 1081, 4096, 8
    sid, vlp = _schedule(spp)
    full, cam, sp = _setup("caustic", W, H, gpu)
    full.path_passes(sid, vlp)
    fc, fn = full.read_radiance()
    full.close()
    acc_c, acc_n = np.zeros_like(fc), np.zeros_like(fn)
    for rank in range(N):
        r, _, _ = _setup("caustic", W, H, gpu)
        r.set_shard(rank, N, 8)
        r.path_passes(sid, vlp)
        assert r.last_streams > 1                        # a 1/8 band uses pass streams
        c, n = r.read_radiance()
        owned = (np.arange(H) // 8) % N == rank
        assert (n[owned] == spp).all() and (n[~owned] == 0).all() and (c[~owned] == 0).all()
        acc_c += c
        acc_n += n
        r.close()
    _same(acc_c, fc, "shard sum colors")
    _same(acc_n, fn, "shard sum counters")
    lp = oracle.light_pass(sp, rnd0, 0)
    ocol, ocnt, _ = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp)   # 8.5 G samples, ~1 min
    _same(fc, ocol, "whole frame vs oracle: colors")
    _same(fn, ocnt, "whole frame vs oracle: counter")


def test_config4_synthetic64_4097_band_8192spp(gpu, rnd0):
    """configs[4] as one GPU of the 8-GPU weak-scaling run renders it (bench.py --workload weak64):
    the 64-sphere synthetic scene at 4097x4097, one 4097x512 band (rank 3 of 8 fixed bands), the
    full 8192 spp -- so vlp_index wraps past LIGHT_POINTS inside the run (pass 8190, SURVEY
    Appendix A.3).  Counters and ownership over the frame; the band's first, middle and last 8-row
    tile bands vs the oracle at the full spp."""
    W, H, spp, N, rank, band = 4097, 4097, 8192, 8, 3, 512
    r, cam, sp = _setup("synthetic64", W, H, gpu)
    assert len(sp) == 64
    r.set_shard(rank, N, band)
    sid, vlp = _schedule(spp)
    assert vlp[8189] == 4095 and vlp[8190] == 0
    r.path_passes(sid, vlp)
    col, cnt = r.read_radiance()
    owned = (np.arange(H) // band) % N == rank
    assert (cnt[owned] == spp).all() and (cnt[~owned] == 0).all()
    assert np.isfinite(col).all() and (col[~owned] == 0).all()
    _pixels_are_toint(r, col)
    lp = oracle.light_pass(sp, rnd0, 0)
    y0 = rank * band
    mid = y0 + band // 2                                   # whole 8-row tile bands: start, middle, end
    for rows in ((y0, y0 + 8), (mid, mid + 8), (y0 + band - 8, y0 + band)):
        ocol, ocnt, _ = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp, rows=rows)
        _same(col[rows[0]:rows[1]], ocol[rows[0]:rows[1]], f"rows {rows}")
        _same(cnt[rows[0]:rows[1]], ocnt[rows[0]:rows[1]], f"rows {rows} counters")
    r.close()


def test_metric_config_cornell_1080p_1024spp(gpu, rnd0):
    """The north star's gate on the metric's own frame: cornell.scn at 1921x1081 (bench.py's
    cornell1080 workload) after 1024 spp.  Whole frame: counters, finiteness and pixel =
    toInt(colors); every 32nd row plus the last (35 rows, 3 % of the frame): colours and counters
    bit for bit against the oracle, and the per-channel L-inf < 1e-3 the north star states
    (`device.cu:544-791`)."""
    W, H, spp = 1921, 1081, 1024
    r, cam, sp = _setup("cornell", W, H, gpu)
    sid, vlp = _schedule(spp)
    r.path_passes(sid, vlp)
    col, cnt = r.read_radiance()
    assert (cnt == spp).all() and np.isfinite(col).all() and (col >= 0).all()
    _pixels_are_toint(r, col)
    lp = oracle.light_pass(sp, rnd0, 0)
    linf = 0.0
    for y in list(range(0, H, 32)) + [H - 1]:
        ocol, ocnt, _ = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp, rows=(y, y + 1))
        linf = max(linf, float(np.abs(col[y].astype(np.float64) - ocol[y].astype(np.float64)).max()))
        _same(col[y], ocol[y], f"row {y}")
        _same(cnt[y], ocnt[y], f"row {y} counters")
    assert linf < 1e-3, linf
    r.close()


def test_north_star_linf_cornell_513_1024spp(gpu, rnd0):
    """The north star's tolerance at a real size: cornell.scn 513x513 (configs[1]'s frame) after
    1024 spp, per-channel L-inf against the CPU path over the whole frame < 1e-3 -- and in fact 0
    (bit-exact).  The pixels are checked as well."""
    W, H, spp = 513, 513, 1024
    r, cam, sp = _setup("cornell", W, H, gpu)
    sid, vlp = _schedule(spp)
    r.path_passes(sid, vlp)
    col, cnt = r.read_radiance()
    lp = oracle.light_pass(sp, rnd0, 0)
    ocol, ocnt, opix = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp)
    linf = float(np.abs(col.astype(np.float64) - ocol.astype(np.float64)).max())
    assert linf < 1e-3, linf
    _same(col, ocol, "colors")
    _same(cnt, ocnt, "counter")
    _same(r.read_pixels(), opix, "pixels")
    r.close()


def test_auto_stream_mode_measures_ten_roles_then_decides(gpu, rnd0, monkeypatch):
    """The auto stream mode's whole sequence on a small frame (cornell 97x65, calls of 8 passes):
    the first ten calls run the ten roles of bdpt_plan.h -- two passes per lane, fused, four per
    lane, the three again with the unpaired fused kernel, pixel pools twice, and twice two per lane
    where the units would run if the frame had the tile workgroups for them -- the eleventh decides,
    and the 96 passes of the twelve calls equal the oracle's bit for bit."""
    for v in ("BDPT_STREAMS_TUNE", "BDPT_POOL", "BDPT_UNITS", "BDPT_MAX_LAUNCH_PASSES"):
        monkeypatch.delenv(v, raising=False)
    W, H, n = 97, 65, 8
    r, cam, sp = _setup("cornell", W, H, gpu)
    sid, vlp = _schedule(12 * n)
    want = [4, 1, 2, 4, 1, 2, 8, 8, 4, 4]
    DECIDED, UNITS = 1, 32                                   # BDPT_CHOICE_* (include/bdpt.h)
    for k in range(12):
        r.path_passes(sid[k * n:(k + 1) * n], vlp[k * n:(k + 1) * n])
        feats = r.last_features
        print(f"call {k + 1}: S = {r.last_streams}, {feats}, choice {r.stream_choice:#x}")
        if k < 10:
            assert r.last_streams == want[k], (k, r.last_streams)
            assert ("pixel_pools" in feats) == (k in (6, 7)), (k, feats)
            assert "unit_fold" not in feats, (k, feats)
            assert r.stream_choice == 0, (k, r.stream_choice)
        else:                                                # decided when the eleventh call was issued
            assert r.stream_choice & DECIDED and not r.stream_choice & UNITS, (k, r.stream_choice)
    col, cnt = r.read_radiance()
    lp = oracle.light_pass(sp, rnd0, 0)
    ocol, ocnt, opix = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp)
    _same(cnt, ocnt, "counter")
    _same(col, ocol, "colors")
    _same(r.read_pixels(), opix, "pixels")
    r.close()


@pytest.mark.parametrize("name", ["cornell", "caustic", "cornell_glass"])
def test_1080p_whole_frame_identical_in_every_kernel_mode(gpu, rnd0, name, monkeypatch):
    """Whole 1921x1081 frames (not sampled rows): the same 128 passes rendered by every kernel
    mode -- the ordered in-kernel fold (units), pixel pools with the sample lists, two and one
    pass(es) per lane with the separate fold, and the fused S = 1 kernel -- are bit-identical over
    every pixel, and the whole frame equals the oracle bit for bit (266 M samples: ~15 s of the
    OpenMP oracle on cornell at 16 threads, a few on caustic).  The modes share the sphere tests
    and shading but differ in everything that maps pixels and passes to lanes, stores radiance and
    folds it; a band-local defect in one of them cannot hide between sampled rows (VERDICT r5 weak
    item 8)."""
    W, H, n = 1921, 1081, 128
    sid, vlp = _schedule(n)
    modes = [("units", 128, {"BDPT_UNITS": "8", "BDPT_POOL": "0"}, "unit_fold"),
             ("pools", 128, {"BDPT_POOL": "64", "BDPT_UNITS": "0"}, "pixel_pools"),
             ("two_per_lane", 64, {"BDPT_POOL": "0", "BDPT_UNITS": "0"}, None),
             ("one_per_lane", 128, {"BDPT_POOL": "0", "BDPT_UNITS": "0"}, None),
             ("fused", 1, {"BDPT_POOL": "0", "BDPT_UNITS": "0"}, None)]
    frames = {}
    for tag, streams, env, feat in modes:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r, cam, sp = _setup(name, W, H, gpu)
        r.set_streams(streams)
        r.path_passes(sid, vlp)
        if feat:
            assert feat in r.last_features, (tag, r.last_features)
        frames[tag] = r.read_radiance()
        r.close()
    ref_col, ref_cnt = frames["units"]
    assert (ref_cnt == n).all()
    for tag, (col, cnt) in frames.items():
        _same(col, ref_col, f"{tag} vs units: colors")
        _same(cnt, ref_cnt, f"{tag} vs units: counter")
    lp = oracle.light_pass(sp, rnd0, 0)
    ocol, ocnt, _ = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp)
    _same(ref_col, ocol, "whole frame vs oracle: colors")
    _same(ref_cnt, ocnt, "whole frame vs oracle: counter")
