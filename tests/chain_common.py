"""Shared by the chain-buffer tests and tests/golden/make_ref_chain_golden.py (not a test module).

The independent statement of include/bdpt.h bdpt_render_chain in numpy float32 (np_chain): the
camera ray, IntersectDevice, the vertex, the mirror and the glass arithmetic, each operation written
out in the header's order.  numpy rounds every elementwise float32 operation once and never
contracts, np.sqrt and / are correctly rounded and denormals are kept, which is the header's
contract.  It calls nothing of the product.  Every comparison the tests make with it is on the bits
of the float32 values; there is no tolerance.

Also here: the probe scene whose path-pass colours pin the chain to the integrator
(probe_chain_scene, probe_chain_colors), the fixtures' loader and the coverage counters."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
RAND_N = 4096 * 1876
DIFF, SPEC, REFR = 0, 1, 2
KIND_DIFFUSE, KIND_EMITTER, KIND_MISS, KIND_EXHAUSTED = range(4)
PLANES = ("id", "first_id", "kind", "bounces", "t", "dp", "position", "normal", "dir", "throughput")
SHARED = ("id", "t", "dp", "position", "normal", "dir")          # the planes render_aov has too
F = np.float32
EPS = F(0.01)                                                    # geom.h:6 EPSILON

SPHERE_DTYPE = np.dtype([("rad", "<f4"), ("p", "<f4", 3), ("e", "<f4", 3), ("c", "<f4", 3), ("refl", "<i4")])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bad = int((bits(a) != bits(b)).sum())
    assert bad == 0, f"{what}: {bad} of {a.size} values differ"


def same_chain(a, b, what, planes=PLANES):
    for k in planes:
        same(a[k], b[k], f"{what}: {k}")


# ---- the statement ---------------------------------------------------------------------------

def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(v):
    """vnorm (vec.h:22): l = 1.f / sqrtf(v.v), each component times l."""
    with np.errstate(divide="ignore", invalid="ignore"):
        l = F(1) / np.sqrt(_dot(v, v))
    return l[..., None] * v


def _vec(a):
    return np.array(a, F).reshape(3)


def camera_rays(cam, W, H, u0, u1):
    """The camera rays of device.cu:562-600 for every pixel, [H, W, 3] origins and directions; u0,
    u1 [H, W] are the jitter randoms.  cam: the 15 floats orig, target, dir, x, y."""
    cam = np.asarray(cam, F).reshape(5, 3)
    orig, cdir, cx, cy = cam[0], cam[2], cam[3], cam[4]
    ux, uy, ud = _unit(cx), _unit(cy), _unit(cdir)
    tx, ty, tz = _dot(_unit(F(-1) * cx), orig), _dot(_unit(F(-1) * cy), orig), _dot(F(-1) * cdir, orig)
    inv_w, inv_h = F(14.0 / W), F(10.5 / H)
    half_w, half_h = np.float64(inv_w * F(W)) / 2.0, np.float64(inv_h * F(H)) / 2.0
    x = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    kx = (((x * inv_w).astype(np.float64) - half_w) + (u0 * inv_w).astype(np.float64)).astype(F)
    ky = (((y * inv_h).astype(np.float64) - half_h) + (u1 * inv_h).astype(np.float64)).astype(F)
    kz = F(10)
    rdir = np.zeros((H, W, 3), F)
    rdir = rdir + kx[..., None] * ux
    rdir = rdir + ky[..., None] * uy
    rdir = rdir + kz * ud
    w = ((tx * kx + ty * ky) + tz * kz) + F(1)
    rdir = (1.0 / w.astype(np.float64)).astype(F)[..., None] * rdir
    return rdir + orig, _unit(rdir)


def closest(sp, o, d):
    """IntersectDevice device.cu:106-124 over rays [m, 3]: the scan from the last sphere down with a
    strict `<`, SphereIntersectDevice's EPSILON rule (:80-104).  -> t [m] (1e20 on a miss), id [m]."""
    t = np.full(len(o), F(1e20))
    idx = np.full(len(o), -1, np.int32)
    p, rad = np.ascontiguousarray(sp["p"], F), np.ascontiguousarray(sp["rad"], F)
    for s in range(len(sp) - 1, -1, -1):
        op = p[s] - o
        b = _dot(op, d)
        det = (b * b - _dot(op, op)) + rad[s] * rad[s]
        with np.errstate(invalid="ignore"):
            root = np.sqrt(det)
        t1, t2 = b - root, b + root
        with np.errstate(invalid="ignore"):
            h = np.where(det < 0, F(0), np.where(t1 > EPS, t1, np.where(t2 > EPS, t2, F(0))))
            take = (h != 0) & (h < t)
        t = np.where(take, h, t)
        idx = np.where(take, np.int32(s), idx)
    return t, idx


def pixel_index(W, H):
    return (np.arange(H, dtype=np.uint32)[:, None] * np.uint32(W) + np.arange(W, dtype=np.uint32)[None, :]).reshape(-1)


def j_index(i, depth, sid):
    """(26 + 25 i + 5 depth + sid) mod (RAND_N - 5) in 32-bit unsigned arithmetic (device.cu:619)."""
    with np.errstate(over="ignore"):
        return (np.uint32(26) + i * np.uint32(25) + np.uint32(5 * depth) + np.uint32(sid)) % np.uint32(RAND_N - 5)


def np_chain(spheres, cam, W, H, rnd=None, sid=0, branch="transmit"):
    """include/bdpt.h bdpt_render_chain for the whole frame.  rnd None: no jitter.  Returns the ten
    planes and, under "_glass" and "_tir", how many glass vertices and total internal reflections
    each pixel's chain passed (for the coverage counters; no part of the interface)."""
    sp = np.ascontiguousarray(spheres)
    n_px = W * H
    i = pixel_index(W, H)
    if rnd is None:
        assert branch == "transmit"
        u0 = u1 = np.zeros((H, W), F)
    else:
        kk = j_index(i, 0, sid)
        u0, u1 = rnd[kk].reshape(H, W), rnd[kk + 1].reshape(H, W)
    o, d = (a.reshape(n_px, 3) for a in camera_rays(cam, W, H, u0, u1))
    o, d = o.copy(), d.copy()
    e, c, p = (np.ascontiguousarray(sp[k], F) for k in ("e", "c", "p"))
    refl = np.ascontiguousarray(sp["refl"])
    emissive = (e != 0).any(axis=1)

    out = {"id": np.full(n_px, -1, np.int32), "first_id": np.full(n_px, -1, np.int32),
           "kind": np.full(n_px, KIND_EXHAUSTED, np.int32), "bounces": np.zeros(n_px, np.int32),
           "t": np.zeros(n_px, F), "dp": np.zeros(n_px, F), "position": np.zeros((n_px, 3), F),
           "normal": np.zeros((n_px, 3), F), "throughput": np.ones((n_px, 3), F),
           "_glass": np.zeros(n_px, np.int32), "_tir": np.zeros(n_px, np.int32)}
    thr = out["throughput"]
    live = np.arange(n_px)
    nc, nt = F(1), F(1.5)
    for depth in range(7):
        if not len(live):
            break
        ol, dl = o[live], d[live]
        t, s = closest(sp, ol, dl)
        if depth == 0:
            out["first_id"][live] = s
        miss = s < 0
        out["kind"][live[miss]] = KIND_MISS
        live, ol, dl, t, s = live[~miss], ol[~miss], dl[~miss], t[~miss], s[~miss]
        out["t"][live] = out["t"][live] + t
        P = ol + t[:, None] * dl
        N = _unit(P - p[s])
        dp = _dot(N, dl)
        nl = (F(-1) * np.where(dp > 0, F(1), F(-1)))[:, None] * N
        stop_e = emissive[s]
        stop_d = ~stop_e & (refl[s] == DIFF)
        stop = stop_e | stop_d
        k = live[stop]
        out["kind"][k] = np.where(stop_e[stop], KIND_EMITTER, KIND_DIFFUSE)
        out["id"][k], out["dp"][k], out["position"][k], out["normal"][k] = s[stop], dp[stop], P[stop], N[stop]
        go = ~stop
        live, dl, s, P, N, nl = live[go], dl[go], s[go], P[go], N[go], nl[go]
        out["bounces"][live] += 1
        R = dl - (F(2) * _dot(N, dl))[:, None] * N
        o[live] = P
        cs = c[s]
        mirror = refl[s] == SPEC
        # glass (every refl but DIFF and SPEC)
        into = _dot(N, nl) > 0
        nnt = np.where(into, nc / nt, nt / nc)
        ddn = _dot(dl, nl)
        cos2t = F(1) - nnt * nnt * (F(1) - ddn * ddn)
        tir = ~mirror & (cos2t < 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            kq = np.where(into, F(1), F(-1)) * (ddn * nnt + np.sqrt(cos2t))
            td = _unit(nnt[:, None] * dl - kq[:, None] * N)
            a, b = nt - nc, nt + nc
            R0 = a * a / (b * b)
            cc = F(1) - np.where(into, -ddn, _dot(td, N))
            Re = R0 + (F(1) - R0) * cc * cc * cc * cc * cc
            Tr = F(1) - Re
            Pp = F(.25) + F(.5) * Re
            RP, TP = Re / Pp, Tr / (F(1) - Pp)
            if branch == "pass":
                reflect = rnd[j_index(i[live], depth, sid) + np.uint32(2)] < Pp
            else:
                reflect = np.zeros(len(live), bool)
            plain = mirror | tir                                   # thr * c, reflect
            kk_ = np.where(reflect, RP, TP)
            thr_glass = (kk_[:, None] * thr[live]) * cs
        thr[live] = np.where(plain[:, None], thr[live] * cs, thr_glass)
        d[live] = np.where((plain | reflect)[:, None], R, td)
        out["_glass"][live] += ~mirror
        out["_tir"][live] += tir
    out["dir"] = d
    res = {}
    for k, v in out.items():
        res[k] = v.reshape((H, W, 3) if v.ndim == 2 else (H, W))
        assert res[k].dtype == (F if k in PLANES[4:] else np.int32), k
    return res


def guide_keys(chain, n):
    """The guide integer of BDPT_DENOISE_THROUGH (include/bdpt.h), -1 where the chain does not end DIFFUSE."""
    b, f, e = (chain[k].astype(np.int64) for k in ("bounces", "first_id", "id"))
    key = np.where(b == 0, e, n + ((b - 1) * n + f) * n + e)
    assert key.max(initial=0) <= 2 ** 31 - 1
    return np.where(chain["kind"] == KIND_DIFFUSE, key, -1).astype(np.int32)


# ---- the probe scene and what its colours say ---------------------------------------------------

def probe_chain_scene(spheres):
    """Every sphere with refl == DIFF or with non-zero e gets the probe emission of
    make_ref_aov_golden.probe_scene, e[s] = (1, s + 1, 0.5 (s + 1) + 0.25); mirrors and glass keep
    e = 0.  One path pass with a zero light-path table then returns the chain's end."""
    from make_ref_aov_golden import probe_emission
    sp = np.ascontiguousarray(spheres).copy()
    ends = (sp["refl"] == DIFF) | (sp["e"] != 0).any(axis=1)
    sp["e"] = np.where(ends[:, None], probe_emission(len(sp)), F(0))
    return sp


def probe_chain_colors(spheres, chain):
    """throughput * (|dp| * e[id]) per channel in the integrator's order (device.cu:651-660), +0 for
    MISS and EXHAUSTED."""
    ended = chain["id"] >= 0
    e = np.ascontiguousarray(spheres["e"], F)[np.where(ended, chain["id"], 0)]
    col = chain["throughput"] * (np.abs(chain["dp"])[..., None] * e)
    assert col.dtype == F
    col[~ended] = 0.0
    return col


# ---- fixtures ---------------------------------------------------------------------------------

def meta():
    return json.load(open(os.path.join(GOLDEN, "ref_chain_meta.json")))


def load_case(name):
    """A committed ref_chain_<name>.npz as the dict the tests use."""
    g = dict(np.load(os.path.join(GOLDEN, f"ref_chain_{name}.npz")))
    g["spheres"] = np.frombuffer(g["spheres"].tobytes(), SPHERE_DTYPE).copy()      # the probe scene
    g["scene_spheres"] = np.frombuffer(g["scene_spheres"].tobytes(), SPHERE_DTYPE).copy()
    g["W"], g["H"] = (int(v) for v in g["size"])
    g["sid"] = int(g["sid"])
    g["table"] = str(g["table"])
    return g


ZERO, CONST = "zero", "const0.875"


def table_of(fx_table, cache, mt607):
    """The random table a fixture names: "zero", "const0.875" or "seed<k>" (mt607(k))."""
    if fx_table not in cache:
        if fx_table == ZERO:
            cache[fx_table] = np.zeros(RAND_N, F)
        elif fx_table == CONST:
            cache[fx_table] = np.full(RAND_N, F(0.875))
        else:
            cache[fx_table] = mt607(int(fx_table[4:]))
    return cache[fx_table]


# ---- coverage counters -------------------------------------------------------------------------

def coverage(chain):
    """What a frame of chains exercises (np_chain's planes, with its "_glass" and "_tir")."""
    ended = chain["id"] >= 0
    return {"pixels": int(chain["id"].size),
            "kinds": [int((chain["kind"] == k).sum()) for k in range(4)],
            "ended_after_bounce": int((ended & (chain["bounces"] >= 1)).sum()),
            "max_bounces": int(chain["bounces"].max()),
            "two_glass": int((chain["_glass"] >= 2).sum()),
            "four_bounces_or_exhausted": int(((chain["bounces"] >= 4) | (chain["kind"] == KIND_EXHAUSTED)).sum()),
            "tir": int(chain["_tir"].sum())}


# ---- rendering with the product (imported lazily: the generator needs none of it) ----------------

_TABLES = {}


def fixture_table(fx):
    import oracle
    return table_of(fx["table"], _TABLES, oracle.mt607)


def camera_of(fx):
    import gpu_bidirectional_raytracer_amd as g
    return g.Camera.from_buffer_copy(np.ascontiguousarray(fx["camera"]).tobytes())


def set_table(r, fx):
    """The fixture's table in the context: generated where a seed names it, uploaded otherwise."""
    if fx["table"].startswith("seed"):
        r.generate_rand(int(fx["table"][4:]))
    else:
        r.write_rand(fixture_table(fx))


def render_case(fx, device, spheres, traversal=None):
    """render_chain of a fixture's inputs with `spheres`, jittered on the fixture's table, under both
    branches -> {"pass": planes, "transmit": planes}."""
    import gpu_bidirectional_raytracer_amd as g
    with g.Renderer(spheres, fx["W"], fx["H"], camera_of(fx), device=device) as r:
        if traversal is not None:
            r.set_traversal(traversal)
        set_table(r, fx)
        return {b: r.render_chain(sid=fx["sid"], branch=b) for b in ("pass", "transmit")}


def statement_case(fx, spheres, branch):
    return np_chain(spheres, fx["camera"], fx["W"], fx["H"], fixture_table(fx), fx["sid"], branch)


def scene(name, W, H):
    import gpu_bidirectional_raytracer_amd as g
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    g.update_camera(cam, W, H)
    return cam, sp


def cam_floats(cam):
    return np.frombuffer(bytes(cam), F).copy()


def schedule(n):
    import gpu_bidirectional_raytracer_amd as g
    s = g.PassScheduler()
    s.light()
    return s.next(n)


def assert_errors(device):
    """The error codes of include/bdpt.h bdpt_render_chain."""
    import pytest
    import gpu_bidirectional_raytracer_amd as g
    E = g._lib
    cam, sp = scene("cornell_mirror", 20, 19)

    def code(call):
        with pytest.raises(g.BdptError) as e:
            call()
        return e.value.code

    with g.Renderer(sp, 20, 19, device=device) as r:
        assert code(lambda: r.render_chain()) == E.BDPT_ESTATE                     # no camera yet
        assert code(lambda: r.last_chain_ms()) == E.BDPT_ESTATE
        r.set_camera(cam)
        assert r.render_chain()["id"].shape == (19, 20)                            # no jitter needs no table
        assert code(lambda: r.render_chain(sid=7)) == E.BDPT_ESTATE                # jitter before a table exists
        assert code(lambda: r.render_chain(sid=7, branch="pass")) == E.BDPT_ESTATE
        assert code(lambda: r.render_chain(branch="pass")) == E.BDPT_EINVAL        # PASS without jitter
        r.generate_rand(15)
        assert code(lambda: r.render_chain(branch="pass")) == E.BDPT_EINVAL
        for bad in (2, -1, "reflect"):
            assert code(lambda: r.render_chain(sid=7, branch=bad)) == E.BDPT_EINVAL, bad
        r.render_chain(sid=g.RAND_N - 1, branch="pass")
        assert code(lambda: r.render_chain(sid=g.RAND_N)) == E.BDPT_EINVAL
        for bad in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (16, 0, 5, 5), (0, 15, 5, 5),
                    (20, 0, 1, 1), (0, 19, 1, 1), (0, 0, 21, 19), (0, 0, 20, 20), (2 ** 31 - 1, 0, 2, 1)):
            assert code(lambda: r.render_chain(window=bad)) == E.BDPT_EINVAL, bad
        assert g.lib.bdpt_render_chain(r._h, 0, 0, 1, 1, 0, 0, 0, None) == E.BDPT_EINVAL   # NULL `out`
        assert r.render_chain(window=(19, 18, 1, 1))["id"].shape == (1, 1)         # the last pixel is inside
        assert list(r.render_chain(planes=("kind", "throughput"))) == ["kind", "throughput"]
        assert r.last_chain_ms() >= 0.0 if device < 0 else r.last_chain_ms() > 0.0


def assert_non_interference(device, name, W, H, streams=None, queued=False):
    """4 passes + render_chain (whole frame and a window, both branches) + 4 passes == 8 passes;
    queued: the first four are not synchronised before the call."""
    import gpu_bidirectional_raytracer_amd as g
    cam, sp = scene(name, W, H)
    sid, vlp = schedule(8)
    got = []
    for probe in (False, True):
        with g.Renderer(sp, W, H, cam, device=device) as r:
            if streams is not None:
                r.set_streams(streams)
            r.light_pass(0)
            r.path_passes(sid[:4], vlp[:4], sync=not (probe and queued))
            if probe:
                r.render_chain(sid=int(sid[0]), branch="pass")
                r.render_chain(window=(3, 2, 9, 5))
            r.path_passes(sid[4:], vlp[4:])
            col, cnt = r.read_radiance()
            got.append((col, cnt, r.read_pixels(), r.read_rand(), r.read_lightpaths()))
    for a, b, what in zip(got[0], got[1], ("colors", "counter", "pixels", "rand", "lightpaths")):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what
    assert (got[0][1] == 8).all()
