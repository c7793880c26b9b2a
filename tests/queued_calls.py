"""Shared by tests/test_gpu_queued_calls.py and tests/test_queued_calls_cpu.py (not a test module):
sequences of calls issued without waiting for the device -- what bench.py and an interactive host
do -- against the oracle chained step by step.  It builds on accum_modes (the mode table, how a mode
is forced and proven) and tiles_common (the masks).

A scenario is a tuple of steps run on one context after light_pass(0):

  ("passes", n, mode, mask[, limit])  path_passes(n passes, sync=False) in accum_modes mode `mode`
                        (or "pool_overlap"), on tiles_common.mask(mask) if mask is not None, cut by
                        BDPT_MAX_LAUNCH_PASSES=limit if given
  ("write", seed)       write_radiance(uneven_state(W, H, seed))
  ("rewind",)           the pass schedule starts over (the next call takes the first sid/vlp again)
  ("reset",)            reset_accum
  ("scene", i, dx)      sphere i moved by dx along x, set_scene
  ("camera", key)       camera_key, update_camera, set_camera
  ("light", cs)         light_pass(cs): a new random table (seed 5 cs) and new light paths
  ("lightpaths", s)     write_lightpaths of the current light paths with rad scaled by s
  ("shard", k, n, band) set_shard
  ("mark",)             noise_mark
  ("estimate", remark)  noise_estimate(remark=remark, pixels=True)
  ("capture",)          history_capture
  ("save", name) / ("load", name)   save_checkpoint / load_checkpoint of <dir>/<name>
  ("update_pixels",)    update_pixels
  ("traversal", mode) / ("specialize", on)   set_traversal / set_specialize
  ("service", name)     denoise, denoise_noise, reproject, preview_denoise, render_aov or pick
  ("read",)             colours, counters, pixels and the products of the steps since the last read
  ("probe",)            calls_in_flight() recorded there (for the tests' evidence; changes nothing)

`run` issues them; with queued=True nothing waits for the device but the reads and the calls that
wait by definition, and Renderer.calls_in_flight() is recorded at every step that is not a "passes"
step: right before a call that blocks the host, right after one that does not.  With queued=False
(the twin) synchronize() follows every step and the frame is read after every "passes" step.
`expect` is the oracle with the same steps applied to its inputs.  Every comparison is on bits."""
import hashlib
import os

import numpy as np

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g
import oracle
import tiles_common as tc
from conftest import SCENES
from denoise_common import np_denoise, to_rgba
from denoise_noise_common import np_denoise_noise
from noise_common import np_noise, same_estimate
from preview_common import np_preview_denoise
from reproject_common import copy_camera, hist_dict, np_reproject

F = np.float32
W, H = 161, 97                       # 6 x 13 tiles, the last column 1 pixel wide, the last row 1 high
# overlapped pools: chunks of 16 x 64 pixels, launches of 128 passes on the two pool streams
POOL_OVERLAP = am.Mode("pool_overlap", 128, pool=16, feature="pixel_pools")
MODES = dict(am.BY_NAME, pool_overlap=POOL_OVERLAP)
SERVICES = ("denoise", "denoise_noise", "reproject", "preview_denoise", "render_aov", "pick")
BLOCKING = {"write", "mark", "estimate", "capture", "save", "load", "service", "lightpaths", "light", "scene",
            "update_pixels"}     # the calls that wait for the device themselves
CPU = -1
MAX_STREAMS = 128                    # BDPT_MAX_STREAMS


def tiles_of(width, height):
    return -(-width // tc.TW), -(-height // tc.TH)


def mask_of(name, width, height):
    return tc.mask(name, *tiles_of(width, height))


def fused(mode, n):
    return mode.last_streams(n) == 1


def passes_launches(step):
    """Launches of a "passes" step (0 for a mask without tiles)."""
    _, n, name, mk = step[:4]
    limit = step[4] if len(step) > 4 else None
    return am.launch_passes(n, limit, fused(MODES[name], n))[1]


class Inputs:
    """What the passes read besides the accumulation -- scene, camera, random table, light paths,
    shard, position in the pass schedule -- kept on the host and changed by the steps, for `run` (which
    must not read them back from a busy device) and for `expect` alike."""

    def __init__(self, scene, width, height, npass):
        self.width, self.height = width, height
        self.cam, self.sp = g.read_scene(os.path.join(SCENES, scene + ".scn"))
        g.update_camera(self.cam, width, height)
        self.seed = 0
        self.rnd = _table(0)
        self.lp = oracle.light_pass(self.sp, self.rnd, 0)
        self.shard = (0, 1, 8)
        self.sid, self.vlp = am.schedule(npass)
        self.p = 0
        self.saved = {}

    def take(self, n):
        s = slice(self.p, self.p + n)
        self.p += n
        return self.sid[s], self.vlp[s]

    def apply(self, step):
        """The host-side part of a step; -> the argument of the Renderer call, where it has one."""
        op = step[0]
        if op == "rewind":
            self.p = 0
        elif op == "scene":
            self.sp = self.sp.copy()
            self.sp["p"][step[1]][0] += F(step[2])
            return self.sp
        elif op == "camera":
            self.cam = copy_camera(self.cam)
            assert g.camera_key(self.cam, step[1])
            g.update_camera(self.cam, self.width, self.height)
            return self.cam
        elif op == "light":
            self.seed = 5 * step[1]
            self.rnd = _table(self.seed)
            self.lp = oracle.light_pass(self.sp, self.rnd, step[1], lp=self.lp)   # entries no path reaches keep their value
        elif op == "lightpaths":
            self.lp = self.lp.copy()
            self.lp["rad"] *= F(step[1])
            return self.lp
        elif op == "shard":
            self.shard = step[1:]
        return None

    def snapshot(self):
        return (self.sp, self.cam, self.seed, self.rnd, self.lp)

    def restore(self, snap):
        self.sp, self.cam, self.seed, self.rnd, self.lp = snap


_TABLES = {}


def _table(seed):
    if seed not in _TABLES:
        _TABLES[seed] = oracle.mt607(seed)
    return _TABLES[seed]


def total_passes(steps):
    """The passes a scenario's schedule must hold: the most any run between rewinds takes."""
    most = cur = 0
    for s in steps:
        if s[0] == "rewind":
            cur = 0
        elif s[0] == "passes":
            cur += s[1]
            most = max(most, cur)
    return most


# ---- running a scenario ---------------------------------------------------------------------------

def arguments(scene, steps, width, height):
    """(inputs at the start, the argument of every step's Renderer call), all computed before
    anything is issued: between two queued calls the host then does nothing but issue them."""
    inp = Inputs(scene, width, height, total_passes(steps))
    start = (inp.sp, inp.cam, inp.lp)
    args = []
    for step in steps:
        arg = inp.apply(step)
        if step[0] == "passes":
            arg = inp.take(step[1]) + (None if step[3] is None else mask_of(step[3], width, height),)
        elif step[0] == "write":
            arg = am.uneven_state(width, height, step[1])
        elif step[0] == "save":
            inp.saved[step[1]] = inp.snapshot()
        elif step[0] == "load":
            inp.restore(inp.saved[step[1]])
        args.append(arg)
    return start, args


def _issue_passes(r, arg, step, monkeypatch, proof):
    """One unsynchronised path_passes call in the step's mode, and the proof that the mode ran from
    the getters that do not synchronise.  The launch count is added to proof["launches"]."""
    import time
    _, n, name, mk = step[:4]
    limit = step[4] if len(step) > 4 else None
    sid, vlp, tiles = arg
    if monkeypatch is None:                                   # the CPU backend: no modes
        r.path_passes(sid, vlp, sync=False, tiles=tiles)
        return
    mode = MODES[name]
    am.force_env(mode, limit, monkeypatch)
    L, launches = am.launch_passes(n, limit, fused(mode, n))
    assert L >= mode.min_launch, f"{name}: launches of {L} passes do not run this mode"
    trav = "bvh" if mode.bvh else "brute"
    if proof.get("specialize") != mode.specialize:            # only on a change: both forget the stream choice
        r.set_specialize(mode.specialize)
    if proof.get("traversal") != trav:
        r.set_traversal(trav)
    proof["specialize"], proof["traversal"] = mode.specialize, trav
    r.set_streams(min(n, MAX_STREAMS) if mode.streams is None else mode.streams)
    if mode.choice is not None:
        r.set_stream_choice(mode.choice)
    r.path_passes(sid, vlp, sync=False, tiles=tiles)
    proof["returned"] = time.perf_counter()
    proof["launches"] += launches if tiles is None or tiles.any() else 0
    what = f"{name}: call of {n} passes, mask {mk}, limit {limit}"
    assert r.last_streams == mode.last_streams(L), f"{what}: last_streams {r.last_streams}"
    if mode.choice is not None:
        assert r.stream_choice == mode.choice, f"{what}: stream_choice {r.stream_choice:#x}"
    feats = r.last_features
    want = "tile_list" if mk is not None else mode.feature
    for f in ("pixel_pools", "unit_fold", "tile_list"):
        assert (f in feats) == (f == want), f"{what}: {feats}"
    assert r.last_specialized == mode.specialize, f"{what}: specialised {r.last_specialized}: {r.specialize_status!r}"
    assert r.last_traversal == ("bvh" if mode.bvh else "brute"), f"{what}: {r.last_traversal}"


def _warm_up(r, steps, args, monkeypatch, width, height):
    """Every distinct call of the scenario once, waited for, then the frame back to zeros.  The first
    use of a kernel in a context builds or loads it, which takes the host longer than the call before
    it takes the device; a scenario must not spend that time between two calls it means to queue."""
    done = set()
    for step, arg in zip(steps, args):
        if step[0] == "passes" and step[1:] not in done and not (step[3] is not None and r.num_devices > 1):
            done.add(step[1:])
            _issue_passes(r, arg, step, monkeypatch, dict(launches=0))
            r.synchronize()
    if done:
        r.write_radiance(np.zeros((height, width, 3), F), np.zeros((height, width), np.uint32))


def _service(r, name):
    if name == "denoise":
        return r.denoise()
    if name == "denoise_noise":
        return r.denoise_noise(variance=True)
    if name == "reproject":
        return r.reproject(weight=True)
    if name == "preview_denoise":
        return r.preview_denoise(weight=True)
    if name == "render_aov":
        return r.render_aov()
    assert name == "pick"
    return r.pick(r.width // 2, r.height // 2)


def run(scene, steps, device, queued, monkeypatch=None, tmpdir=None, width=W, height=H, devices=None):
    """-> dict(reads=[...], in_flight=[(step index, step, calls in flight)], launches=(expected,
    counted), frames=[state after every "passes" step; the twin only]).  A read is a dict of colors,
    counter, pixels and the products since the last read, by name: mark, estimate, history,
    checkpoint (the file's bytes), service (its result) and guides (the first hit, with a service)."""
    (sp, cam, lp), args = arguments(scene, steps, width, height)
    out = dict(reads=[], in_flight=[], frames=[])
    proof = dict(launches=0)
    products = {}
    gpu = device != CPU
    kw = dict(devices=devices) if devices is not None else dict(device=device)
    with g.Renderer(sp, width, height, cam, **kw) as r:
        r.light_pass(0)
        if gpu:
            same_bytes(r.read_lightpaths(), lp, "the light paths of light_pass(0) vs the oracle's")
            _warm_up(r, steps, args, monkeypatch, width, height)
            r.kernel_timing(reset=True)
        for k, (step, arg) in enumerate(zip(steps, args)):
            op = step[0]
            if op not in ("passes", "read", "probe", "rewind") and queued and op in BLOCKING:
                out["in_flight"].append((k, step, r.calls_in_flight()))
            if op == "passes":
                _issue_passes(r, arg, step, monkeypatch if gpu else None, proof)
            elif op == "write":
                r.write_radiance(*arg)
            elif op == "reset":
                r.reset_accum()
            elif op == "scene":
                r.set_scene(arg)
            elif op == "camera":
                r.set_camera(arg)
            elif op == "light":
                r.light_pass(step[1])
            elif op == "lightpaths":
                r.write_lightpaths(arg)
            elif op == "shard":
                r.set_shard(*step[1:])
            elif op == "mark":
                r.noise_mark()
                products["mark"] = None                       # read at the next "read"
            elif op == "estimate":
                products["estimate"] = r.noise_estimate(remark=bool(step[1]), pixels=True)
                products["mark"] = None
            elif op == "capture":
                r.history_capture()
                products["history"] = None
            elif op == "save":
                r.save_checkpoint(os.path.join(tmpdir, step[1]))
                products["checkpoint"] = open(os.path.join(tmpdir, step[1]), "rb").read()
            elif op == "load":
                r.load_checkpoint(os.path.join(tmpdir, step[1]))
            elif op == "update_pixels":
                r.update_pixels()
            elif op == "traversal":
                r.set_traversal(step[1])
                proof["traversal"] = step[1]
            elif op == "specialize":
                r.set_specialize(bool(step[1]))
                proof["specialize"] = bool(step[1])
            elif op == "service":
                products["service"] = _service(r, step[1])
            elif op == "read":
                col, cnt = r.read_radiance()
                rd = dict(colors=col, counter=cnt, pixels=r.read_pixels())
                if "mark" in products:
                    products["mark"] = r.noise_read_mark()
                if "history" in products:
                    products["history"] = r.history_read()
                if "service" in products:
                    products["guides"] = r.render_aov()
                rd.update(products)
                products = {}
                out["reads"].append(rd)
            elif op == "probe":
                out["in_flight"].append((k, step, r.calls_in_flight()))
            elif op != "rewind":
                raise AssertionError(f"unknown step {step}")
            if op not in ("passes", "read", "probe", "rewind") and queued and op not in BLOCKING:
                out["in_flight"].append((k, step, r.calls_in_flight()))
            if not queued:
                r.synchronize()
                if op == "passes":
                    out["frames"].append(tc.read_state(r))
        if gpu and steps[-1][0] == "read":                    # (kernel_timing waits; a run that ends queued closes so)
            out["launches"] = (proof["launches"], r.kernel_timing()[1])
    return out


# ---- the oracle -----------------------------------------------------------------------------------

_CALLS = {}


def _digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.digest()


def oracle_call(inp, sid, vlp, state, rows):
    """oracle.path_passes over `rows` (a tuple of (y0, y1) ranges, None: the frame) from `state`;
    computed once per input."""
    key = (inp.width, inp.height, rows, _digest(inp.sp, bytes(inp.cam), np.uint32(inp.seed), inp.lp, sid, vlp, *state))
    if key not in _CALLS:
        col, cnt, px = state
        for r in (rows if rows is not None else ((0, inp.height),)):
            col, cnt, px = oracle.path_passes(inp.sp, inp.rnd, inp.cam, inp.width, inp.height, inp.lp, sid, vlp,
                                              colors=col, counter=cnt, pixels=px, rows=r)
        _CALLS[key] = (col, cnt, px)
    return _CALLS[key]


def _shard_rows(shard, height, rows):
    """The row ranges a call renders: the shard's bands, cut to `rows` (single rows) if given."""
    k, n, band = shard
    own = [y for y in range(height) if (y // band) % n == k]
    if rows is not None:
        return tuple((y, y + 1) for y in rows if y in own)
    if n == 1:
        return None
    return tuple((y0, min(y0 + band, height)) for y0 in range(0, height, band) if (y0 // band) % n == k)


_EXPECTED = {}


def expect(scene, steps, rows=None, width=W, height=H):
    """-> (reads, frames), computed once per input: frames are the states (colors, counter, pixels)
    after every "passes" step, reads the states at every "read" step as dicts of colors, counter and
    pixels -- and, with rows=None, the products the oracle can state: mark (colours, counts) and
    estimate (np_noise's dict).  With rows=(y, ...) only those rows of the frame are computed and
    meaningful.  A mask is applied as tiles_common.chain applies it: the unmasked result where the
    mask says, the state before elsewhere."""
    key = (scene, steps, rows, width, height)
    if key not in _EXPECTED:
        _EXPECTED[key] = _expect(scene, steps, rows, width, height)
    return _EXPECTED[key]


def _expect(scene, steps, rows, width, height):
    inp = Inputs(scene, width, height, total_passes(steps))
    state = (np.zeros((height, width, 3), F), np.zeros((height, width), np.uint32), np.zeros((height, width, 4), np.uint8))
    mark = (np.zeros((height, width, 3), F), np.zeros((height, width), np.uint32))
    saved, reads, frames, products = {}, [], [], {}
    for step in steps:
        op = step[0]
        inp.apply(step)
        col, cnt, px = state
        if op == "passes":
            sid, vlp = inp.take(step[1])
            rr = _shard_rows(inp.shard, height, rows)
            ocol, ocnt, opx = oracle_call(inp, sid, vlp, state, rr)
            if step[3] is not None:                           # as tiles_common.chain selects
                m = tc.pixel_mask(mask_of(step[3], width, height), width, height)
                ocol, ocnt, opx = np.where(m[..., None], ocol, col), np.where(m, ocnt, cnt), np.where(m[..., None], opx, px)
            state = (ocol, ocnt, opx)
            frames.append(state)
        elif op == "write":
            col, cnt = am.uneven_state(width, height, step[1])
            state = (col, cnt, to_rgba(col))
        elif op == "reset":
            state = (col, np.zeros_like(cnt), px)
        elif op == "save":
            saved[step[1]] = (state, inp.snapshot())
        elif op == "load":
            (col, cnt, _), snap = saved[step[1]]
            inp.restore(snap)
            state = (col, cnt, to_rgba(col))
        elif op == "mark":
            mark = (col.copy(), cnt.copy())
            products["mark"] = mark
        elif op == "estimate" and rows is None:
            est = np_noise(col, cnt, mark[0], mark[1], remark=bool(step[1]))
            mark = est["mark"]
            products["estimate"], products["mark"] = est, mark
        elif op == "read":
            reads.append(dict(colors=state[0], counter=state[1], pixels=state[2], **(products if rows is None else {})))
            products = {}
        if op in ("write", "reset", "scene", "camera", "load"):   # they clear the mark
            mark = (mark[0], np.zeros_like(mark[1]))
    return reads, frames


# ---- comparing ------------------------------------------------------------------------------------

def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bad = np.argwhere((a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))).any(-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:4].tolist()}"


def same_frame(got, want, what, rows=None):
    """colors, counter and pixels of two reads, on all rows or on `rows`."""
    for k in ("colors", "counter", "pixels"):
        a, b = got[k], want[k]
        if rows is not None:
            a, b = a[list(rows)], b[list(rows)]
        am.same(np.ascontiguousarray(a), np.ascontiguousarray(b), f"{what}: {k}")


def same_product(a, b, what):
    """Two products of the same kind (arrays, tuples or dicts of them, numbers, bytes)."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), f"{what}: {sorted(a)} vs {sorted(b)}"
        for k in a:
            same_product(a[k], b[k], f"{what}[{k}]")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_product(x, y, f"{what}[{i}]")
    elif isinstance(a, np.ndarray):
        same_bytes(a, b, what)
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), f"{what}: {a!r} vs {b!r}"
    else:
        assert a == b, f"{what}: {a!r} vs {b!r}"


def same_reads(got, want, what, rows=None):
    """Every read of two runs: frames and every product both hold."""
    assert len(got) == len(want), f"{what}: {len(got)} reads vs {len(want)}"
    for k, (a, b) in enumerate(zip(got, want)):
        same_frame(a, b, f"{what}: read {k + 1}", rows)
        for name in a:
            if name == "estimate" and name in b:
                same_estimate(a[name], b[name], f"{what}: read {k + 1}: estimate")
            elif name in b and name not in ("colors", "counter", "pixels"):
                same_product(a[name], b[name], f"{what}: read {k + 1}: {name}")


def check_service(name, read, frame, mark, hist, inp_sp):
    """A service's result in `read` against its numpy statement on `frame` = (colors, counter,
    pixels) the service saw, `mark` = (mc, mn) or None and `hist` = hist_dict(...) or None."""
    col, cnt, _ = frame
    res, aov, refl = read["service"], read["guides"], inp_sp["refl"]
    if name == "denoise":
        same_bytes(res, np_denoise(col, aov["id"], aov["normal"], refl), "denoise vs numpy")
    elif name == "denoise_noise":
        wcol, wvar = np_denoise_noise(col, cnt, mark, aov["id"], aov["normal"], refl)
        same_bytes(res[0], wcol, "denoise_noise vs numpy: colours")
        same_bytes(res[1], wvar, "denoise_noise vs numpy: variance")
    elif name == "reproject":
        o, w, _ = np_reproject(col, cnt, aov, refl, hist)
        same_bytes(res[0], o, "reproject vs numpy: colours")
        same_bytes(res[1], w, "reproject vs numpy: weight")
    elif name == "preview_denoise":
        o, a, _ = np_preview_denoise(col, cnt, aov, refl, hist)
        same_bytes(res[0], o, "preview_denoise vs numpy: colours")
        same_bytes(res[1], a, "preview_denoise vs numpy: count")
    elif name == "pick":
        cy, cx = aov["id"].shape[0] // 2, aov["id"].shape[1] // 2
        assert res[0] == int(aov["id"][cy, cx]), f"pick: sphere {res[0]} vs the first hit's {aov['id'][cy, cx]}"
        assert F(res[1]).tobytes() == F(aov["t"][cy, cx]).tobytes(), "pick: distance vs the first hit's"


def drained(in_flight):
    """The steps at which no call was in flight, as a message ('' when there is none)."""
    bad = [f"the queue had drained before {step}; nothing was tested" for _, step, n in in_flight if n < 1]
    return "; ".join(bad)


# ---- the scenarios --------------------------------------------------------------------------------
# ("probe",) is the one step that exists for the tests alone: calls_in_flight() right there.

# the mode set: (mode, mask); masks only with modes that may run on a tile list
M = (("fused_paired", None), ("two_per_lane", None), ("four_per_lane", None), ("one_per_lane", None), ("pool2", None),
     ("pool_overlap", None), ("units3", None), ("precompiled_one_per_lane", None), ("one_per_lane", "A"),
     ("fused_paired", "B"))
M_BVH = (("bvh_fused", None), ("bvh_one_per_lane", None), ("bvh_one_per_lane", "A"))
A_SET = (("pool_overlap", None), ("two_per_lane", None), ("units3", None), ("one_per_lane", "A"))
ROWS = (0, 48, 96)


def label(entry):
    return entry[0] + ("" if entry[1] is None else f"[{entry[1]}]")


def pairs(a, n1, n2, modes=M):
    """One context: for every B of `modes`, the same uneven start, A's call, a probe, B's call, a
    probe (2 there: A was still running when B's call had been issued), a read."""
    steps = []
    for b in modes:
        steps += [("write", 7), ("rewind",), ("passes", n1, a[0], a[1]), ("probe",), ("passes", n2, b[0], b[1]), ("probe",), ("read",)]
    return tuple(steps)


def ring(n):
    """More calls than ring slots (2 kRing + 3 = 11) from an uneven start, every base mode of M, five
    masked calls with another tile list each time (A, B, C, F, A), one call cut into four launches of
    five passes -- the first, so that the counters that start just below the cap cross it in
    different launches -- a probe after every call, one read.  The fused calls and the units are the
    long ones (a fused call of n passes takes ten times a pass-stream call's time): they are placed
    so that every short call is issued while one of them runs or waits, whatever the host's pace."""
    calls = (("two_per_lane", None, 20, 6), ("fused_paired", None, n), ("one_per_lane", "A", n), ("fused_paired", "B", n),
             ("four_per_lane", None, n), ("one_per_lane", "C", n), ("pool2", None, n), ("fused_paired", "F", n),
             ("pool_overlap", None, 2 * n), ("precompiled_one_per_lane", "A", n), ("units3", None, n))
    steps = [("write", 7)]
    for c in calls:
        steps += [("passes", c[2], c[0], c[1]) + tuple(c[3:]), ("probe",)]
    return tuple(steps + [("read",)])


def passes_per_pixel(steps, width, height):
    """How many passes every pixel was rendered for: the sum over the calls whose mask holds it."""
    n = np.zeros((height, width), np.int64)
    for s in steps:
        if s[0] == "passes":
            n += s[1] if s[3] is None else s[1] * tc.pixel_mask(mask_of(s[3], width, height), width, height)
    return n


OPS = (("write", 3), ("reset",), ("scene", 6, -5.0), ("camera", "a"), ("light", 3), ("lightpaths", 0.5),
       ("shard", 0, 2, 16), ("mark",), ("estimate", 1), ("capture",), ("save", "queued.ckpt"), ("load", "start.ckpt"),
       ("update_pixels",), ("traversal", "auto"), ("specialize", 0)) + tuple(("service", s) for s in SERVICES)
# (index into A_SET, op): a sharded context takes no tile mask, so no shard change behind a masked call
CASES = tuple((k, op) for op in OPS for k, a in enumerate(A_SET) if not (op[0] == "shard" and a[1] is not None))
SETUP = 8                                                     # passes before the mark, history and checkpoint of a prefix


def op_label(op):
    return "-".join(str(x) for x in op).replace(".", "_")


def behind(a, op, b, n1, n2):
    """A's call, the op queued behind it, B's call, a read; where the op needs something to work on,
    a short synchronous prefix makes it: a mark and a history SETUP passes old, or a checkpoint."""
    pre = ()
    if op[0] == "estimate" or op[0] == "service":
        pre = (("passes", SETUP, "fused_paired", None), ("mark",), ("capture",), ("read",))
    elif op[0] == "load":
        pre = (("passes", SETUP, "fused_paired", None), ("save", op[1]), ("read",))
    if op == ("specialize", 0):
        b = ({"fused_paired": "precompiled_fused", "one_per_lane": "precompiled_one_per_lane"}[b[0]], b[1])
    return pre + (("passes", n1, a[0], a[1]), op, ("passes", n2, b[0], b[1]), ("read",))


# ---- how long A's call must be (GPU) --------------------------------------------------------------
# The passes of A's call, chosen from a measurement so that the call's device time is at least ten
# times the host time from its return to the probe (profiles/queued_calls_sizing.json, DESIGN.md
# "Queued calls"): 1024 on cornell for every mode (the smallest ratio is 111, the masked one_per_lane
# call), one value so that the unmasked chains share their oracle calls, and 256 on synthetic64 (197),
# where the oracle is slower.  N1 overrides by label; N2 is B's call.
N1_DEFAULT, N1_BVH, N2 = 1024, 256, 64
N_RING, N_GROUP = 256, 256           # the calls of the ring scenario and of the group's
N1 = {}


def n1_of(entry):
    return N1.get(label(entry), N1_BVH if entry[0].startswith("bvh_") else N1_DEFAULT)


def measure(entry, device, monkeypatch, scene, n1):
    """One unsynchronised call of n1 passes in the mode from an uneven start -> dict(mode, n1,
    device_ms of the call, issue_us the host took to issue it, probe_us from path_passes' return to
    the probe's answer (what a scenario does in between: the getters that prove the mode), in_flight
    the probe's answer)."""
    import time
    step = ("passes", n1, entry[0], entry[1])
    (sp, cam, _), (arg,) = arguments(scene, (step,), W, H)
    state0 = am.uneven_state(W, H, 7)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        for timed in (False, True):                           # once to build and load the kernels
            r.write_radiance(*state0)
            r.path_timing(reset=True)
            proof = dict(launches=0)
            t0 = time.perf_counter()
            _issue_passes(r, arg, step, monkeypatch, proof)    # the call and the getters that prove its mode
            n = r.calls_in_flight()
            t2 = time.perf_counter()
            ms = r.path_timing()[0]
    return dict(mode=label(entry), scene=scene, n1=n1, device_ms=ms, issue_us=(proof["returned"] - t0) * 1e6,
                probe_us=(t2 - proof["returned"]) * 1e6, in_flight=n)
