"""Shared by tests/test_gpu_accum_state.py and tests/test_accum_state_cpu.py (not a test module):
every kernel mode of the path integrator -- how to force it and how to prove afterwards that it
ran -- and scenarios that start from an accumulation state that differs from pixel to pixel, cut a
call into several launches, or change the shard and reset the frame between calls.  A scenario is
run through a Renderer (`run`) and through the oracle chained call by call (`expect`); every
comparison is on the bits of the values, with no tolerance."""
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import gpu_bidirectional_raytracer_amd as g
import oracle
from conftest import SCENES

CAP = g.COUNTER_CAP
W, H = 97, 65                       # 3 x 32 + 1 columns, 8 x 8 + 1 rows: both packed edges
DECIDED, FUSED, PAIRED, QUARTER = 1, 2, 4, 8          # BDPT_CHOICE_* (include/bdpt.h)
# the uncapped pixels' counters: the assign branch of the running mean (0), young pixels, pixels
# that cross the cap in the first call of 9 passes (29991, 29995, 29999) and in the second of 11
# (29985), in different ranges of 3 passes, one that ends at 29999 after 20 passes (29979), and
# one above the cap, which `counter < 30000` leaves alone
CYCLE = (0, 1, 2, 7, 29979, 29985, 29991, 29995, 29999, 30001)


def _ceil(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Mode:
    """One kernel mode: `streams` for set_streams, `choice` for set_stream_choice (auto mode only),
    the BDPT_POOL / BDPT_UNITS values, and what the context must report after a call.
    streams=None: one stream per pass of the call (pools and units take their launch shape from it)."""
    name: str
    streams: Optional[int]
    choice: Optional[int] = None
    pool: int = 0
    units: int = 0
    specialize: bool = True
    bvh: bool = False
    feature: Optional[str] = None
    per_lane: int = 0               # passes per lane of a launch of L passes (0: not by this rule)
    min_launch: int = 1             # launches below this many passes do not run the mode

    def last_streams(self, L):
        """last_streams after a call whose launches have L passes (the first launch's count)."""
        if self.streams == 1 or (self.choice is not None and self.choice & FUSED):
            return 1
        if self.per_lane:
            return _ceil(L, self.per_lane)
        if self.streams is not None and self.streams > 1:
            return min(self.streams, L)
        return L


MODES = [
    Mode("fused_paired", 0, DECIDED | FUSED | PAIRED),
    Mode("fused_unpaired", 0, DECIDED | FUSED),
    Mode("two_per_lane", 0, DECIDED, per_lane=2, min_launch=4),
    Mode("four_per_lane", 0, DECIDED | QUARTER, per_lane=4, min_launch=8),
    Mode("one_per_lane", -1),
    Mode("fixed_s3", 3),
    Mode("pool2", None, pool=2, feature="pixel_pools"),
    Mode("pool4", None, pool=4, feature="pixel_pools"),
    Mode("units3", None, units=3, feature="unit_fold"),
    Mode("precompiled_fused", 1, specialize=False),
    Mode("precompiled_one_per_lane", -1, specialize=False),
    Mode("bvh_fused", 1, specialize=False, bvh=True),
    Mode("bvh_one_per_lane", -1, specialize=False, bvh=True),
]
BY_NAME = {m.name: m for m in MODES}


def uneven_state(width, height, seed):
    """(colors0 [H, W, 3] float32, counter0 [H, W] uint32).  With q the row-major pixel index,
    counter0 = 30000 where q % 150 < 100: runs of 100 pixels at the cap, longer than a wave's 64
    and shorter than a pool chunk of 128 or 256, starting at every even residue mod 64 over the
    frame.  The other pixels cycle through CYCLE.  colors0 is seeded, in [0, 4), with a few exact
    zeros (whole pixels and single channels); the channels differ."""
    n = width * height
    q = np.arange(n)
    capped = q % 150 < 100
    counter = np.full(n, CAP, np.uint32)
    counter[~capped] = np.asarray(CYCLE, np.uint32)[np.arange(int((~capped).sum())) % len(CYCLE)]
    rng = np.random.default_rng(seed)
    colors = rng.random((n, 3), dtype=np.float32) * np.float32(4.0)
    colors[::53] = 0.0              # whole pixels (capped and uncapped ones)
    colors.reshape(-1)[::211] = 0.0  # single channels
    return colors.reshape(height, width, 3), counter.reshape(height, width)


def closed_form_counter(counter0, npass):
    """The counter after npass passes: one increment per pass while it is below the cap."""
    c0 = counter0.astype(np.int64)
    return np.where(c0 >= CAP, c0, np.minimum(c0 + npass, CAP)).astype(np.uint32)


@dataclass(frozen=True)
class Scenario:
    """Steps after light_pass(0): ("write", seed) = write_radiance(uneven_state(W, H, seed)),
    ("shard", k, n, band), ("reset",) and ("passes", n).  limit = BDPT_MAX_LAUNCH_PASSES."""
    name: str
    scene: str
    steps: Tuple[tuple, ...]
    limit: Optional[int] = None
    width: int = W
    height: int = H

    @property
    def npass(self):
        return sum(s[1] for s in self.steps if s[0] == "passes")


def uneven(scene):
    return Scenario("uneven", scene, (("write", 7), ("passes", 9), ("passes", 11)))


def split(npass=20, limit=6, scene="cornell"):
    return Scenario(f"split{npass}x{limit}", scene, (("passes", npass),), limit=limit)


def uneven_split(scene="cornell"):
    return Scenario("uneven_split", scene, (("write", 7), ("passes", 20)), limit=6)


def state_changes(scene="cornell"):
    return Scenario("state_changes", scene,
                    (("shard", 1, 3, 8), ("passes", 5), ("shard", 0, 1, 8), ("passes", 7), ("reset",), ("passes", 4)))


def launch_passes(npass, limit, fused):
    """(passes of the first launch, launches) of a call, as bdpt_path_passes cuts it: at most 128
    passes (64 for the fused kernel) or `limit`, in equal launches."""
    chunk = 64 if fused else 128
    if limit is not None:
        chunk = min(chunk, limit)
    n = _ceil(npass, chunk)
    return _ceil(npass, n), n


def load_scene(sc):
    cam, sp = g.read_scene(os.path.join(SCENES, sc.scene + ".scn"))
    g.update_camera(cam, sc.width, sc.height)
    return cam, sp


def schedule(n):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


def force_env(mode, limit, monkeypatch):
    """The environment of a mode: BDPT_POOL and BDPT_UNITS always set ("0" where unused)."""
    monkeypatch.setenv("BDPT_POOL", str(mode.pool))
    monkeypatch.setenv("BDPT_UNITS", str(mode.units))
    if limit is None:
        monkeypatch.delenv("BDPT_MAX_LAUNCH_PASSES", raising=False)
    else:
        monkeypatch.setenv("BDPT_MAX_LAUNCH_PASSES", str(limit))


def _call(r, mode, sid, vlp, limit):
    """One path_passes call in `mode`, with the proof that the mode ran and how it was cut."""
    n = len(sid)
    if mode is None:                                          # the CPU backend: no modes
        r.path_passes(sid, vlp)
        return
    fused = mode.last_streams(n) == 1
    L, launches = launch_passes(n, limit, fused)
    assert L >= mode.min_launch, f"{mode.name}: launches of {L} passes do not run this mode"
    r.set_streams(n if mode.streams is None else mode.streams)
    if mode.choice is not None:        # forgotten after a scene, shard, traversal or stream-mode change
        r.set_stream_choice(mode.choice)
    r.kernel_timing(reset=True)
    r.path_passes(sid, vlp)
    what = f"{mode.name}: call of {n} passes, limit {limit}"
    assert r.kernel_timing(reset=True)[1] == launches, f"{what}: not {launches} launches"
    assert r.last_streams == mode.last_streams(L), f"{what}: last_streams {r.last_streams}"
    if mode.choice is not None:
        assert r.stream_choice == mode.choice, f"{what}: stream_choice {r.stream_choice:#x}"
    if mode.feature:
        assert mode.feature in r.last_features, f"{what}: {r.last_features}"
    for other in ("pixel_pools", "unit_fold"):
        if other != mode.feature:
            assert other not in r.last_features, f"{what}: {r.last_features}"
    assert r.last_specialized == mode.specialize, f"{what}: specialised {r.last_specialized}: {r.specialize_status!r}"
    assert r.last_traversal == ("bvh" if mode.bvh else "brute"), f"{what}: {r.last_traversal}"


def run(mode, scenario, device, monkeypatch=None):
    """The scenario on `device` in `mode` (None on the CPU backend) -> [(colors, counter, pixels)]:
    the state after light_pass and every "write" (pixels as the context holds them then) and
    after every "passes" step, in step order."""
    if mode is not None:
        force_env(mode, scenario.limit, monkeypatch)
    cam, sp = load_scene(scenario)
    sid, vlp = schedule(scenario.npass)
    out, p = [], 0
    with g.Renderer(sp, scenario.width, scenario.height, cam, device=device) as r:
        if mode is not None:
            r.set_specialize(mode.specialize)
            if mode.bvh:
                assert r.has_bvh
                r.set_traversal("bvh")
        r.light_pass(0)

        def state():
            col, cnt = r.read_radiance()
            out.append((col, cnt, r.read_pixels()))

        if scenario.steps[0][0] != "write":
            state()
        for step in scenario.steps:
            if step[0] == "write":
                r.write_radiance(*uneven_state(scenario.width, scenario.height, step[1]))
                state()
            elif step[0] == "shard":
                r.set_shard(*step[1:])
            elif step[0] == "reset":
                r.reset_accum()
            else:
                _call(r, mode, sid[p:p + step[1]], vlp[p:p + step[1]], scenario.limit)
                p += step[1]
                state()
    return out


_EXPECTED = {}


def expect(scenario, state0):
    """The oracle chained call by call from state0 = (colors, counter, pixels), the first state
    `run` returns: write_radiance recomputes the pixels, so the chain starts from the pixels the
    context holds, not from zeros.  A sharded step is chained over the shard's own rows only.
    Returns the states after every "passes" step.  Computed once per scenario and start."""
    key = (scenario,) + tuple(np.ascontiguousarray(a).tobytes() for a in state0)
    if key in _EXPECTED:
        return _EXPECTED[key]
    cam, sp = load_scene(scenario)
    rnd = oracle.mt607(0)
    lp = oracle.light_pass(sp, rnd, 0)
    sid, vlp = schedule(scenario.npass)
    col, cnt, px = (np.array(a) for a in state0)
    shard, out, p = (0, 1, 8), [], 0
    Hh, Ww = scenario.height, scenario.width
    for step in scenario.steps:
        if step[0] == "shard":
            shard = step[1:]
        elif step[0] == "reset":
            cnt = np.zeros_like(cnt)
        elif step[0] == "passes":
            k, n, band = shard
            for y0 in range(0, Hh, band):
                if (y0 // band) % n != k:
                    continue
                col, cnt, px = oracle.path_passes(sp, rnd, cam, Ww, Hh, lp, sid[p:p + step[1]], vlp[p:p + step[1]],
                                                  colors=col, counter=cnt, pixels=px, rows=(y0, min(y0 + band, Hh)))
            p += step[1]
            out.append((col, cnt, px))
    _EXPECTED[key] = out
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bad = np.argwhere(bits(a) != bits(b))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first at {bad[:4].tolist()}"


def check(scenario, got, what):
    """`got` (from run) against the oracle, and the two invariants that need no oracle: the
    closed-form counter, and pixels that start at or above the cap keep colours and pixel bytes."""
    want = expect(scenario, got[0])
    assert len(got) == len(want) + 1
    col0, cnt0, px0 = got[0]
    plain = all(s[0] in ("write", "passes") for s in scenario.steps)      # no shard change, no reset
    done, k = 0, 0
    for step in scenario.steps:
        if step[0] != "passes":
            continue
        done += step[1]
        (col, cnt, px), (ocol, ocnt, opx) = got[k + 1], want[k]
        tag = f"{what}: after call {k + 1} ({done} passes)"
        print(f"{tag}: {int((bits(col) != bits(ocol)).sum())} colour values, {int((cnt != ocnt).sum())} counters, "
              f"{int((px != opx).any(-1).sum())} pixels differ from the oracle")
        if plain:
            same(cnt, closed_form_counter(cnt0, done), f"{tag}: counter vs the closed form")
            held = cnt0 >= CAP
            same(col[held], col0[held], f"{tag}: colours of pixels at the cap")
            same(px[held], px0[held], f"{tag}: pixel bytes of pixels at the cap")
        same(cnt, ocnt, f"{tag}: counter")
        same(col, ocol, f"{tag}: colors")
        same(px, opx, f"{tag}: pixels")
        k += 1
