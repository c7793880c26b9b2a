"""Shared by tests/test_follow_cpu.py and tests/test_gpu_follow.py (not a test module): the numpy
statement of the sphere-following history (include/bdpt.h bdpt_history_follow).  It
is reproject_common.np_reproject itself, fed first-hit planes whose `position` is
position - delta[clip(id, 0)]: the one change the definition makes.  Besides: the followable rule
and the offsets restated in numpy, the cases (a history of 4 passes under the scene's camera and
the unmoved spheres, a frame of one pass under the moved ones), the conditions that keep a case from
passing vacuously, and the runs both backends share.  Every comparison is on the bits of the float32
values; there is no tolerance."""
import functools

import numpy as np

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, schedule
from denoise_common import eligible
from preview_common import DEFAULTS as PREVIEW_DEFAULTS
from preview_common import np_preview_levels
from reproject_common import CPU, DEFAULTS, F, SWEEP, hist_dict, history_of, moved, np_reproject

NONE, SAME, MOVED, UNUSABLE = 0, 1, 2, 3                      # BDPT_HISTORY_*

# (scene, W, H, traversal of the first hits, ((sphere, sphere keys), ...), camera keys)
CASES = [
    ("cornell_diff", 65, 49, None, ((6, "6"),), ()),
    ("cornell_diff", 65, 49, None, ((7, "9"),), ()),
    ("cornell_diff", 65, 49, None, ((6, "444444"),), ()),
    ("cornell_diff", 40, 33, None, ((6, "66"), (7, "4")), ()),          # two offsets
    ("cornell_diff", 40, 33, None, ((6, "6"),), ("a",)),                # and a camera move
    ("synthetic64", 40, 33, None, ((48, "6"),), ()),                    # a sphere index >= 32
    ("complex", 40, 33, "brute", ((159, "6"),), ()),                    # a 783-entry table
    ("complex", 40, 33, "bvh", ((159, "6"),), ()),
    ("cornell_diff", 7, 5, None, ((6, "6"),), ()),                      # one workgroup, partial tiles
    ("cornell_diff", 129, 3, None, ((7, "9"),), ()),
]
# the three cases that also carry the conditions against a vacuous pass
BIG = CASES[:3]


def case_id(case):
    name, W, H, traversal, moves, camkeys = case
    return "-".join([name, f"{W}x{H}"] + ([traversal] if traversal else []) +
                    [f"s{k}k{keys}" for k, keys in moves] + list(camkeys))


def state_of(S0, S):
    """The followable rule of include/bdpt.h on two sphere arrays (a history is stored)."""
    if len(S0) != len(S):
        return UNUSABLE
    if S0.tobytes() == S.tobytes():
        return SAME
    for a, b in zip(S0, S):
        if any(a[f].tobytes() != b[f].tobytes() for f in ("rad", "e", "c", "refl")):
            return UNUSABLE
        if not (b["e"] == 0).all() and a["p"].tobytes() != b["p"].tobytes():
            return UNUSABLE
    return MOVED


def offsets(S0, S):
    """delta[k] = S[k].p - S0[k].p in float32, +0 where the components compare equal."""
    a, b = np.ascontiguousarray(S0["p"], F), np.ascontiguousarray(S["p"], F)
    d = np.where(b == a, F(0), b - a)
    assert d.dtype == F
    return d


def moved_spheres(sp, moves):
    sp = sp.copy()
    for k, keys in moves:
        for key in keys:
            assert g.sphere_key(sp, k, key)
    return sp


def shifted(aov, delta):
    """The first-hit planes with P' = P - delta[id1] in place of P."""
    out = dict(aov)
    out["position"] = (np.ascontiguousarray(aov["position"], F) - delta[np.clip(aov["id"], 0, None)]).astype(F)
    return out


def np_follow(colors, counter, aov, refl, hist, delta, **prm):
    """The definition with follow on in state 2."""
    return np_reproject(colors, counter, shifted(aov, delta), refl, hist, **prm)


@functools.lru_cache(maxsize=None)
def inputs_of(case):
    """Rendered on the CPU backend once per case and never modified: dict of cam0, S0, the 4-pass
    history (hc, hm) and its first hit aov0, S1, cam1, the one-pass frame (col, cnt) under them, its
    first hit aov1, delta."""
    name, W, H, traversal, moves, camkeys = case
    cam0, S0, hc, hm, aov0 = history_of(name, W, H)
    S1 = moved_spheres(S0, moves)
    cam1 = moved(cam0, camkeys, W, H)
    sid, vlp = schedule(1)
    with g.Renderer(S1, W, H, cam1, device=CPU) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        col, cnt = r.read_radiance()
        aov1 = r.render_aov()
    assert state_of(S0, S1) == MOVED
    return dict(cam0=cam0, S0=S0, hc=hc, hm=hm, aov0=aov0, S1=S1, cam1=cam1, col=col, cnt=cnt, aov1=aov1,
                delta=offsets(S0, S1), moved_ids=[k for k, _ in moves])


def statement(case, prm, shift=True):
    """(out, weight, taps) of the numpy statement (shift=False: of a kernel that forgets the shift)."""
    i = inputs_of(case)
    hist = hist_dict(i["cam0"], i["hc"], i["hm"], i["aov0"])
    delta = i["delta"] if shift else np.zeros_like(i["delta"])
    return np_follow(i["col"], i["cnt"], i["aov1"], i["S1"]["refl"], hist, delta, **prm)


def assert_not_vacuous(case):
    """On the statement itself, with the defaults: some pixel of a moved sphere takes history; for the
    65x49 cases at least 30 do, at least 10 eligible static pixels take none (what the sphere used to
    hide), and at least 20 moved-sphere pixels differ from the result without the shift."""
    i = inputs_of(case)
    o, w, taps = statement(case, DEFAULTS)
    o0, w0, taps0 = statement(case, DEFAULTS, shift=False)
    on = np.isin(i["aov1"]["id"], i["moved_ids"])
    static = eligible(i["aov1"]["id"], i["S1"]["refl"], "diffuse") & ~on
    with_history = int((on & (taps > 0)).sum())
    uncovered = int((static & (taps == 0)).sum())
    differ = int((on & ((o.view(np.uint32) != o0.view(np.uint32)).any(axis=-1) |
                        (w.view(np.uint32) != w0.view(np.uint32)))).sum())
    print(f"{case_id(case)}: on sphere {int(on.sum())}, with history {with_history}, with 1-3 taps "
          f"{int((on & (taps > 0) & (taps < 4)).sum())}, uncovered {uncovered}, differ from the unshifted {differ}, "
          f"unshifted with history {int((on & (taps0 > 0)).sum())}")
    assert with_history >= 1
    if case in BIG:
        assert with_history >= 30 and uncovered >= 10 and differ >= 20
    return on


def setup(r, case):
    """The history written while the context holds S0, then the moved spheres and the frame."""
    i = inputs_of(case)
    r.set_scene(i["S0"])
    r.history_write(i["cam0"], i["hc"], i["hm"])
    r.set_scene(i["S1"])
    r.write_radiance(i["col"], i["cnt"])


def renderer(device, case):
    name, W, H, traversal, moves, camkeys = case
    i = inputs_of(case)
    r = g.Renderer(i["S0"], W, H, i["cam1"], device=device)
    if traversal:
        r.set_traversal(traversal)
    return r


def results(device, case, params=SWEEP):
    """Per parameter set: reproject (out, weight), then the capture's history_read; then the denoised
    preview at levels = 0 and at the defaults.  Follow is on."""
    res = []
    i = inputs_of(case)
    with renderer(device, case) as r:
        r.history_follow(True)
        for prm in params:
            setup(r, case)
            state, delta = r.history_motion()
            assert state == MOVED
            same(delta, i["delta"], "history_motion: delta")
            assert r.history_info()[0] is True
            res.append(r.reproject(weight=True, **prm))
            r.history_capture(**prm)
            assert r.history_motion()[0] == SAME
            res.append(r.history_read())
        setup(r, case)
        res.append(r.preview_denoise(weight=True, levels=0))
        res.append(r.preview_denoise(weight=True))
        same(r.read_radiance()[0], i["col"], "the accumulation is only read")
    return res


def want(case, params=SWEEP):
    """The statement's counterpart of results()."""
    i = inputs_of(case)
    out = []
    for prm in params:
        o, w, _ = statement(case, prm)
        out += [(o, w), (o, w)]
    o, w, _ = statement(case, DEFAULTS)
    out.append((o, w))
    p = PREVIEW_DEFAULTS
    out.append(np_preview_levels(o, w, i["aov1"]["id"], i["aov1"]["normal"], i["S1"]["refl"], p["levels"],
                                 p["normal_power"], p["sigma_color"], p["count_ref"], p["materials"]))
    return out


def what_of(case, k, params=SWEEP):
    n = 2 * len(params)
    if k < n:
        return f"{case_id(case)} {params[k // 2]} {'capture' if k % 2 else 'reproject'}"
    return f"{case_id(case)} preview_denoise {'defaults' if k > n else 'levels=0'}"


def assert_equal_results(got, ref, case, who, params=SWEEP):
    assert len(got) == len(ref)
    for k, ((a, aw), (b, bw)) in enumerate(zip(got, ref)):
        same(a, b, f"{who}: {what_of(case, k, params)}: colours")
        same(aw, bw, f"{who}: {what_of(case, k, params)}: weight")
