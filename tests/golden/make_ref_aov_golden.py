"""Regenerate the reference-produced fixtures of the first-hit feature buffers,
tests/golden/ref_aov_<case>.npz and ref_aov_meta.json (run from the repo root, on a machine that
has the reference tree, after `make`):

    python tests/golden/make_ref_aov_golden.py

The reference has no feature buffers, but its path kernel exposes the first hit when every sphere
of a scene is an emitter and dev_lp is zero: one pass of RadiancePathTracingKernel then ends at the
first sphere the camera ray meets and returns, per channel, e[id] * fabs(dp) (device.cu:651-660
with throughput == 1), or +0 on a miss.  With the probe emission

    e[s] = (1, s + 1, 0.5 * (s + 1) + 0.25)

colors.x is |dp| bit for bit and colors.y / colors.x is s + 1, so the reference's colours pin the
sphere index and |dp| of every pixel -- and with them the camera ray, the closest hit, the hit point
and the normal that dp is formed from.  Everything stored here comes from oracle/_ref/libref.so (the
reference's own device.cu as host C++, oracle/ref.py), one pass with fresh counters, through the
table of ref.mt607(15) or, for the unjittered rays, an all-zero table (both camera randoms +0.0f).

Each ref_aov_<case>.npz holds the inputs as make_ref_golden.py stores them (the probe spheres as
raw bytes of SPHERE_DTYPE, camera as 15 floats, size, sid) with the table's seed (-1: the zero
table; never the table) and the reference's colours whole.  tests/test_aov_cpu.py and
tests/test_gpu_aov.py compare e[id] * |dp| of render_aov with them, with no tolerance.

The comparison is meaningful only if a hit and a miss cannot be confused: the generator asserts
that every pixel of every case is either all-zero (a miss) or has colors.x > 0.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402
from make_golden import read_scene_py  # noqa: E402
from make_ref_golden import RAND_N, SCENES, W20, H19, wrap_sids  # noqa: E402

TABLE_SEED = 15
ZERO_TABLE = -1                 # table_seed of the cases whose table is all zeros (no jitter)


def probe_emission(n):
    """e[s] = (1, s + 1, 0.5 * (s + 1) + 0.25): exact in float32 for every sphere count in use."""
    s1 = np.arange(1, n + 1, dtype=np.float32)
    return np.stack([np.ones(n, np.float32), s1, np.float32(0.5) * s1 + np.float32(0.25)], axis=1)


def probe_scene(sp):
    """The scene with every sphere an emitter of the probe emission (geometry and materials kept)."""
    sp = sp.copy()
    sp["e"] = probe_emission(len(sp))
    return sp


def _case(name, scene, W, H, sid, table_seed=TABLE_SEED, note=""):
    orig, target, sp = read_scene_py(os.path.join(SCENES, scene + ".scn"))
    return {"name": name, "scene": scene, "W": W, "H": H, "sid": int(sid), "table_seed": int(table_seed),
            "spheres": probe_scene(sp), "camera": oracle.update_camera(orig, target, W, H), "note": note}


def cases():
    wrap = wrap_sids(W20, H19)
    return [
        _case("cornell", "cornell", W20, H19, 7, note="closed box: every pixel hits"),
        _case("cornell_glass", "cornell_glass", W20, H19, 7, note="glass and mirror spheres are hits like any other"),
        _case("caustic", "caustic", W20, H19, 7, note="open scene: misses"),
        _case("cornell_nojitter", "cornell", W20, H19, 7, table_seed=ZERO_TABLE,
              note="all-zero table: the unjittered ray of render_aov(sid=None)"),
        _case("cornell_33x9", "cornell", 33, 9, 7, note="a wide frame, another inv_width / inv_height"),
        _case("cornell_wrap", "cornell", W20, H19, wrap[0],
              note="kk = (26 + 25 i + sid) mod (rand_count - 5) wraps inside the frame (device.cu:562)"),
        _case("cornell_sid_last", "cornell", W20, H19, RAND_N - 1, note="sid = RAND_N - 1: every pixel wrapped once"),
        _case("complex", "complex", W20, H19, 7, note="783 spheres (BVH scene), 30 of them visible, and misses"),
    ]


def table_of(case, lib, tables):
    seed = case["table_seed"]
    if seed not in tables:
        tables[seed] = np.zeros(RAND_N, np.float32) if seed == ZERO_TABLE else lib.mt607(seed)
    return tables[seed]


def run_reference(case, lib, rnd):
    """One pass of the reference's path kernel over the probe scene with zero dev_lp -> colours."""
    lp = np.zeros(oracle.LIGHT_POINTS, oracle.LIGHTPATH_DTYPE)
    col, cnt, _ = lib.path_passes(case["spheres"], rnd, case["camera"], case["W"], case["H"], lp,
                                  [case["sid"]], [1])
    assert (cnt == 1).all()
    hit = col[..., 0] > 0
    assert (col[~hit] == 0).all() and not np.signbit(col[~hit]).any(), \
        f"{case['name']}: a pixel is neither a miss (all +0) nor a hit (colors.x > 0)"
    return col


def fixture_arrays(case, colors):
    return {"spheres": np.frombuffer(np.ascontiguousarray(case["spheres"]).tobytes(), np.uint8),
            "camera": case["camera"].view(np.float32).reshape(-1),
            "size": np.array([case["W"], case["H"]], np.int32),
            "sid": np.uint32(case["sid"]), "table_seed": np.int32(case["table_seed"]),
            "colors": colors}


def decode(colors):
    """(id, |dp|) the reference's colours encode: id = colors.y / colors.x - 1, -1 on a miss."""
    hit = colors[..., 0] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(hit, colors[..., 1] / colors[..., 0], np.float32(0))
    return np.where(hit, np.rint(ratio).astype(np.int32) - 1, -1), colors[..., 0]


def load_case(name):
    """A committed fixture as the dict the tests use (no reference, no library needed)."""
    g = dict(np.load(os.path.join(HERE, f"ref_aov_{name}.npz")))
    g["spheres"] = np.frombuffer(g["spheres"].tobytes(), oracle.SPHERE_DTYPE).copy()
    g["W"], g["H"] = (int(v) for v in g["size"])
    g["sid"], g["table_seed"] = int(g["sid"]), int(g["table_seed"])
    return g


def main():
    from oracle import ref as R
    lib = R.ref()
    tables, meta = {}, {"rand_n": RAND_N, "zero_table": ZERO_TABLE, "cases": []}
    for case in cases():
        col = run_reference(case, lib, table_of(case, lib, tables))
        path = os.path.join(HERE, f"ref_aov_{case['name']}.npz")
        np.savez_compressed(path, **fixture_arrays(case, col))
        ids, _ = decode(col)
        meta["cases"].append({"name": case["name"], "scene": case["scene"], "size": [case["W"], case["H"]],
                              "sid": case["sid"], "table_seed": case["table_seed"],
                              "spheres": int(len(case["spheres"])), "hit_pixels": int((ids >= 0).sum()),
                              "spheres_seen": int(len(np.unique(ids[ids >= 0]))), "note": case["note"]})
        print(f"{case['name']:18s} {os.path.getsize(path):6d} B  hits {int((ids >= 0).sum()):4d} of {ids.size}  "
              f"spheres seen {len(np.unique(ids[ids >= 0]))}")
    with open(os.path.join(HERE, "ref_aov_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
