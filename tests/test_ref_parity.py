"""The oracle, the committed fixtures and the CPU backend against the reference's own code.

oracle/_ref/libref.so is the reference's src/device.cu and src/MersenneTwister_kernel.cu compiled
in place as host C++ (Makefile "The reference build", oracle/ref_shim.h, oracle/ref_driver.cpp,
oracle/ref.py), with cos/sin/pow of a float evaluated as (float)f((double)x), the project's
floating-point contract.  Everything the suite otherwise proves is "equal to oracle/bdpt_oracle.c",
our restatement; this module holds the restatement, the fixtures the GPU tests read and the
product's CPU backend to the reference's own program text.  Every comparison is exact: floats are
compared as their uint32 bit patterns, there is no tolerance.

Skipped only where neither the library nor the reference tree (BDPT_REFERENCE) exists.  No GPU.
"""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, SCENES
from oracle import ref as R

if not R.available():
    pytest.skip("no reference build (oracle/_ref/libref.so) and no reference tree", allow_module_level=True)

import gpu_bidirectional_raytracer_amd as g  # noqa: E402
import make_ref_golden as mrg  # noqa: E402
from make_golden import read_scene_py  # noqa: E402
from test_gpu_fuzz import random_large_scene, random_scene  # noqa: E402
from test_gpu_ref_fixtures import run_renderer  # noqa: E402

META = json.load(open(os.path.join(GOLDEN, "render_meta.json")))
KA = json.load(open(os.path.join(GOLDEN, "known_answers.json")))
ALL_SCENES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(SCENES, "*.scn")))
CASES = {c["name"]: c for c in mrg.cases()}
RAND_N = oracle.RAND_N


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def lp_bits(lp):
    return u32(mrg.lp_rows(lp))


@pytest.fixture(scope="module")
def lib():
    return R.ref()


@pytest.fixture(scope="module")
def ref_table(lib):
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = lib.mt607(seed)
            cache[seed].setflags(write=False)
        return cache[seed]
    return get


@pytest.fixture(scope="module")
def ref_results(lib, ref_table):
    """Every edge case through the reference, once, shared by the tests below."""
    cache = {}

    def get(name):
        if name not in cache:
            c = CASES[name]
            cache[name] = mrg.run_reference(c, lib, ref_table(c["current_sample"] * 5))
        return cache[name]
    return get


def assert_frame_equal(got, want, what):
    """(lp, colors, counter, pixels) of two runs, bit for bit."""
    assert np.array_equal(lp_bits(got[0]), lp_bits(want[0])), \
        f"{what}: {int((lp_bits(got[0]) != lp_bits(want[0])).any(axis=1).sum())} dev_lp entries differ"
    assert np.array_equal(got[2], want[2]), f"{what}: counters differ"
    bad = int((u32(got[1]) != u32(want[1])).sum())
    assert bad == 0, f"{what}: {bad} of {want[1].size} radiance values differ"
    assert np.array_equal(got[3], want[3]), f"{what}: pixels differ"


def both(lib, sp, rnd, cam, W, H, sid, vlp, current_sample=0, colors0=None, counter0=None):
    olp = oracle.light_pass(sp, rnd, current_sample)
    o = oracle.path_passes(sp, rnd, cam, W, H, olp, sid, vlp, colors=colors0, counter=counter0)
    rlp = lib.light_pass(sp, rnd, current_sample, cam=cam, width=W, height=H)
    r = lib.path_passes(sp, rnd, cam, W, H, rlp, sid, vlp, colors=colors0, counter=counter0)
    return (olp,) + tuple(o), (rlp,) + tuple(r)


# ---- the random table -----------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 5, 15])
def test_table_equals_reference(ref_table, seed):
    """All 7,684,096 entries of RandomGPU (MersenneTwister_kernel.cu:63-110); 15 is the
    current_sample*5 seed of a re-initialisation at sample 3."""
    assert same_bits(oracle.mt607(seed), ref_table(seed))


def test_mt607_fixture_and_record_equal_reference(ref_table):
    gold = np.load(os.path.join(GOLDEN, "mt607.npz"))
    for seed in (0, 5):
        t = ref_table(seed)
        assert same_bits(t[gold["idx"]], gold[f"seed{seed}"])
        assert oracle.fnv1a64(t) == int(gold[f"fnv_seed{seed}"])
        assert f"{oracle.fnv1a64(t):016x}" == KA["reference_build"]["fnv1a64_table"][str(seed)]
    assert f"{oracle.fnv1a64(ref_table(15)):016x}" == KA["reference_build"]["fnv1a64_table"]["15"]
    for k, v in KA["d_rand_seed0"].items():
        assert ref_table(0)[int(k)] == np.float32(v)


# ---- the committed oracle-written fixtures become pins ---------------------------------------

@pytest.mark.parametrize("name", META["scenes"])
def test_render_fixture_equals_reference(lib, ref_table, name):
    """lp, colors, counter and pixels of render_<name>.npz, which the GPU tests read, from the
    same inputs through the reference's light pass and path kernel."""
    gold = np.load(os.path.join(GOLDEN, f"render_{name}.npz"))
    W, H = META["internal_size"]
    _, _, sp = read_scene_py(os.path.join(SCENES, name + ".scn"))
    cam = gold["camera"].view(oracle.CAMERA_DTYPE)
    rnd = ref_table(0)
    lp = lib.light_pass(sp, rnd, 0, cam=cam, width=W, height=H)
    col, cnt, px = lib.path_passes(sp, rnd, cam, W, H, lp, META["sid"], META["vlp"])
    assert same_bits(mrg.lp_rows(lp), gold["lp"])
    assert same_bits(col, gold["colors"])
    assert same_bits(cnt, gold["counter"])
    assert same_bits(px, gold["pixels"])


# ---- the oracle on every scene file and on the fuzz scenes ------------------------------------

@pytest.mark.parametrize("size", [(33, 25), (20, 19)], ids=["33x25", "20x19"])
@pytest.mark.parametrize("name", ALL_SCENES)
def test_oracle_equals_reference_on_scene(lib, ref_table, name, size):
    W, H = size
    orig, target, sp = read_scene_py(os.path.join(SCENES, name + ".scn"))
    cam = oracle.update_camera(orig, target, W, H)
    o, r = both(lib, sp, ref_table(0), cam, W, H, META["sid"], META["vlp"])
    assert_frame_equal(o, r, f"{name} {W}x{H}")
    assert (r[2] == META["npass"]).all()


def _fuzz(lib, rnd, cam, sp, npass, what):
    from test_cpu_fuzz import H, W
    g.update_camera(cam, W, H)
    s = g.PassScheduler()
    s.light()
    sid, vlp = s.next(npass)
    o, r = both(lib, sp, rnd, oracle.camera_array(cam), W, H, sid, vlp)
    assert_frame_equal(o, r, what)


def test_oracle_equals_reference_on_random_scenes(lib, ref_table):
    """The seeds of test_cpu_fuzz.py (zero to three emitters, every material, cameras in and out)."""
    from test_gpu_fuzz import NPASS, SEEDS
    for seed in range(SEEDS):
        cam, sp = random_scene(1000 + seed)
        _fuzz(lib, ref_table(0), cam, sp, NPASS, f"random_scene({1000 + seed})")


def test_oracle_equals_reference_on_random_large_scenes(lib, ref_table):
    from test_gpu_fuzz import SEEDS
    for seed in range(max(6, SEEDS // 8)):
        cam, sp = random_large_scene(2000 + seed)
        _fuzz(lib, ref_table(0), cam, sp, 3, f"random_large_scene({2000 + seed})")


# ---- edges the earlier pins never touched -----------------------------------------------------

def test_wrap_sid_arithmetic():
    """The wrap case does what its name says, from the index formulas alone (device.cu:562,619):
    kk falls back to the table's start between two neighbouring pixels of the frame, j falls back
    between two depths of one path, every read stays inside the table, and RAND_N-1 is there."""
    c = CASES["wrap_sid"]
    n = c["W"] * c["H"]
    sids = [int(s) for s in c["sid"]]
    assert sids[-1] == RAND_N - 1 and all(0 <= s < RAND_N for s in sids)
    m = RAND_N - 5
    for s in sids[:-1]:
        kk = [mrg.kk_index(i, s) for i in range(n)]
        drops = [i for i in range(1, n) if kk[i] < kk[i - 1]]
        assert len(drops) == 1 and 0 < drops[0] < n - 1, (s, drops)
    depth_wraps = set()
    for s in sids:
        for i in range(n):
            assert 26 + 25 * i + 5 * 6 + s < 2 ** 32
            j = [mrg.j_index(i, d, s) for d in range(7)]
            assert max(j) + 4 < RAND_N and mrg.kk_index(i, s) + 1 < RAND_N     # j+2 .. j+4: device.cu:479,670
            depth_wraps |= {d for d in range(1, 7) if j[d] < j[d - 1]}
    assert {3, 5} <= depth_wraps
    assert any(m - 5 < mrg.j_index(i, d, s) for s in sids for i in range(n) for d in range(7))
    # the light pass never reaches its modulus (device.cu:173,273, seed_id = 0, ind < 4096)
    assert 3 * 5 + 4095 * 4 < RAND_N - 4 and 4095 * 154 + 4 < RAND_N - 3
    assert CASES["light_cs3"]["current_sample"] == 3
    assert 4095 in CASES["vlp4095"]["vlp"]
    assert (CASES["one_pixel"]["W"], CASES["one_pixel"]["H"]) == (1, 1)
    cap = CASES["cap"]
    assert cap["colors0"].min() > 0 and set(np.unique(cap["counter0"])) == {0, 7, 29998, 29999}
    assert int(CASES["no_emitter"]["spheres"]["e"].any(axis=1).sum()) == 0
    assert int(CASES["three_emitters"]["spheres"]["e"].any(axis=1).sum()) == 3


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_reference_on_edge_case(ref_table, ref_results, name):
    c = CASES[name]
    rnd = ref_table(c["current_sample"] * 5)
    lp = oracle.light_pass(c["spheres"], rnd, c["current_sample"])
    o = oracle.path_passes(c["spheres"], rnd, c["camera"], c["W"], c["H"], lp, c["sid"], c["vlp"],
                           colors=c["colors0"], counter=c["counter0"])
    r = ref_results(name)
    assert_frame_equal((lp,) + tuple(o), (r["lp"], r["colors"], r["counter"], r["pixels"]), name)


def test_cap_case_stops_at_30000(ref_results):
    c, r = CASES["cap"], ref_results("cap")
    want = np.minimum(c["counter0"].astype(np.int64) + len(c["sid"]), 30000)
    assert np.array_equal(r["counter"], want) and (r["counter"] == 30000).any()


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_backend_equals_reference_on_edge_case(ref_table, ref_results, name):
    """The product itself (Renderer on the host-CPU backend, csrc/bdpt_cpu.cpp), table included."""
    c, r = CASES[name], ref_results(name)
    got = run_renderer(c, device=-1)
    assert_frame_equal((got["lp"], got["colors"], got["counter"], got["pixels"]),
                       (r["lp"], r["colors"], r["counter"], r["pixels"]), name)


def test_cpu_backend_table_seed15_equals_reference(ref_table):
    c = CASES["light_cs3"]
    cam = g.Camera.from_buffer_copy(c["camera"].tobytes())
    with g.Renderer(c["spheres"], c["W"], c["H"], cam, device=-1) as r:
        r.generate_rand(15)
        assert same_bits(r.read_rand(), ref_table(15))


# ---- the reference-written fixtures of the GPU tests ------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_ref_fixture_regenerates(ref_results, name):
    """Regenerating tests/golden/ref_<name>.npz reproduces the committed bytes of every array."""
    want = mrg.fixture_arrays(CASES[name], ref_results(name))
    have = np.load(os.path.join(GOLDEN, f"ref_{name}.npz"))
    assert sorted(have.files) == sorted(want)
    for k, v in want.items():
        assert same_bits(np.asarray(v), have[k]), f"ref_{name}.npz[{k}]"


def test_ref_rand_fixture_and_meta_regenerate(lib):
    want = mrg.rand_fixture(lib)
    have = np.load(os.path.join(GOLDEN, "ref_mt607.npz"))
    assert sorted(have.files) == sorted(want)
    for k, v in want.items():
        assert same_bits(np.asarray(v), have[k]), k
    meta = json.load(open(os.path.join(GOLDEN, "ref_meta.json")))
    assert [c["name"] for c in meta["cases"]] == list(CASES)
    for m in meta["cases"]:
        c = CASES[m["name"]]
        assert m["sid"] == c["sid"].tolist() and m["vlp"] == c["vlp"].tolist()
        assert m["size"] == [c["W"], c["H"]] and m["current_sample"] == c["current_sample"]
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"ref_{name}.npz")) <= 102400


# ---- the second build: platform float cos/sin/pow ---------------------------------------------

def test_platform_libm_build_keeps_table_and_counters(ref_table):
    """The build whose cos/sin/pow are the platform's float overloads differs from the correctly
    rounded one in a minority of radiance values (measured in DESIGN.md "Oracle"); what must not
    depend on libm is the table (no libm call) and the counters."""
    lm = R.ref_libm()
    assert same_bits(lm.mt607(5), ref_table(5))
    W, H = META["internal_size"]
    for name in META["scenes"]:
        gold = np.load(os.path.join(GOLDEN, f"render_{name}.npz"))
        _, _, sp = read_scene_py(os.path.join(SCENES, name + ".scn"))
        cam = gold["camera"].view(oracle.CAMERA_DTYPE)
        lp = lm.light_pass(sp, ref_table(0), 0, cam=cam, width=W, height=H)
        _, cnt, _ = lm.path_passes(sp, ref_table(0), cam, W, H, lp, META["sid"], META["vlp"])
        assert same_bits(cnt, gold["counter"])


# ---- the host functions: display_func.c against the oracle and the product's C-ABI ------------
# libref_host.so is the reference's display_func.c compiled as C behind empty GL/CUDA stand-ins
# (oracle/ref_stubs/).  ReInit/ReInitScene are counting stubs there, so a key only moves the camera
# or a sphere; the tests re-derive the camera (UpdateCamera) themselves, as ReInit does.

CAMERA_KEYS = ["a", "d", "w", "s", "r", "f", "left", "right", "up", "down", "page_up", "page_down"]
SPHERE_KEYS = ["4", "+", "6", "+", "8", "-", "2", "-", "-", "9", "+", "3", "+", "+", "4", "9"]


def _abi_camera(cam):
    return g.Camera.from_buffer_copy(np.ascontiguousarray(cam).tobytes())


@pytest.fixture(scope="module")
def host():
    return R.ref_host()


@pytest.mark.parametrize("name", ALL_SCENES)
def test_read_scene_and_update_camera_equal_reference(host, name):
    """ReadScene (display_func.c:112-175) and UpdateCamera (:177-190) at two frame sizes."""
    path = os.path.join(SCENES, name + ".scn")
    rcam, rsp = host.read_scene(path)
    orig, target, sp = read_scene_py(path)
    acam, asp = g.read_scene(path)
    assert same_bits(rsp, sp.astype(oracle.SPHERE_DTYPE)), "read_scene_py"
    assert same_bits(rsp, asp.astype(oracle.SPHERE_DTYPE)), "bdpt_read_scene"
    assert same_bits(rcam["orig"][0], orig) and same_bits(rcam["target"][0], target)
    assert same_bits(rcam, oracle.camera_array(acam))
    for W, H in ((33, 25), (641, 481), (20, 19)):
        want = host.update_camera(W, H)
        assert same_bits(want, oracle.update_camera(orig, target, W, H)), f"oracle {W}x{H}"
        assert same_bits(want, oracle.camera_array(g.update_camera(acam, W, H))), f"C-ABI {W}x{H}"


@pytest.mark.parametrize("name", ALL_SCENES)
def test_camera_keys_equal_reference(host, name):
    """KeyFunc a d w s r f (display_func.c:291-334) and SpecialFunc's arrows and page keys
    (:384-433), each from the camera the previous key and UpdateCamera left, so the moves compound."""
    W, H = 33, 25
    host.read_scene(os.path.join(SCENES, name + ".scn"))
    want = host.update_camera(W, H)
    ocam = want.copy()
    acam = _abi_camera(want)
    for key in CAMERA_KEYS:
        reinit, reinit_scene = host.key(key)
        assert (reinit, reinit_scene) == (1, 0), key
        want = host.camera()
        moved = oracle.special_key(ocam, key) if key in oracle.GLUT_SPECIAL else oracle.key_camera(ocam, key)
        assert moved and g.camera_key(acam, key), key
        assert same_bits(want, ocam), f"oracle after {key}"
        assert same_bits(want, oracle.camera_array(acam)), f"C-ABI after {key}"
        want = host.update_camera(W, H)                      # ReInit -> UpdateCamera (smallpt_cpu.c:382)
        oracle.lib.oracle_update_camera(ctypes.c_void_p(ocam.ctypes.data), W, H)
        g.update_camera(acam, W, H)
        assert same_bits(want, ocam), f"oracle UpdateCamera after {key}"
        assert same_bits(want, oracle.camera_array(acam)), f"C-ABI UpdateCamera after {key}"


@pytest.mark.parametrize("name", ALL_SCENES)
def test_sphere_keys_equal_reference(host, name):
    """KeyFunc + - (display_func.c:335-346) and 4 6 8 2 9 3 (:347-370): the selected sphere and
    the sphere list after every key, against bdpt_sphere_key and SmallPT.KeyFunc's selection rule."""
    _, sp = host.read_scene(os.path.join(SCENES, name + ".scn"))
    sp = sp.astype(g.SPHERE_DTYPE)
    n, cur = len(sp), 0
    assert host.current_sphere == 0
    for key in SPHERE_KEYS:
        reinit, reinit_scene = host.key(key)
        assert (reinit, reinit_scene) == (0, 1), key
        if key in "+-":
            cur = (cur + (1 if key == "+" else n - 1)) % n        # SmallPT.KeyFunc
        else:
            assert g.sphere_key(sp, cur, key), key
        assert host.current_sphere == cur
        assert same_bits(host.spheres(), sp.astype(oracle.SPHERE_DTYPE)), f"after {key}"
