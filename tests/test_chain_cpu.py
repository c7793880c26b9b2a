"""Chain buffers (include/bdpt.h bdpt_render_chain) on the CPU backend (device = BDPT_DEVICE_CPU,
csrc/bdpt_cpu.cpp bdpt_cpu_render_chain); runs without a GPU.

Three independent witnesses, all compared on float32 bits with no tolerance: the numpy statement of
the definition (tests/chain_common.py np_chain), the reference's own path kernel on the probe scenes
(tests/golden/ref_chain_*.npz, written by make_ref_chain_golden.py), and one oracle path pass."""
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
import make_ref_chain_golden as mrc
import oracle
from chain_common import (CONST, KIND_DIFFUSE, KIND_EMITTER, KIND_EXHAUSTED, KIND_MISS, PLANES, SHARED, assert_errors,
                          assert_non_interference, bits, cam_floats, camera_of, coverage, fixture_table, load_case, meta,
                          np_chain, probe_chain_colors, render_case, same, same_chain, scene, set_table, statement_case)
from conftest import GOLDEN
from make_ref_golden import wrap_sids
from oracle import ref as R

CPU = -1
META = meta()
CASES = [c["name"] for c in META["cases"]]


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.fixture(scope="module")
def rendered():
    """Every fixture through the CPU backend once: the probe scene and the scene's own spheres."""
    os.environ.setdefault("BDPT_CPU_THREADS", "4")
    out = {}
    for name in CASES:
        fx = load_case(name)
        out[name] = (fx, render_case(fx, CPU, fx["spheres"]), render_case(fx, CPU, fx["scene_spheres"]))
    return out


@pytest.mark.parametrize("name", CASES)
def test_equals_the_statement_on_all_planes(rendered, name):
    fx, probe, own = rendered[name]
    for branch in ("pass", "transmit"):
        same_chain(probe[branch], statement_case(fx, fx["spheres"], branch), f"{name} probe {branch}")
        same_chain(own[branch], statement_case(fx, fx["scene_spheres"], branch), f"{name} {branch}")
        assert sorted(own[branch]) == sorted(PLANES)


@pytest.mark.parametrize("name", CASES)
def test_probe_colours_equal_the_reference(rendered, name):
    fx, probe, _ = rendered[name]
    same(probe_chain_colors(fx["spheres"], probe["pass"]), fx["colors"], f"{name}: throughput * (|dp| * e[id])")


@pytest.mark.parametrize("name", ["mirror_s15", "glass_const", "hall_s15", "mirror_zero", "complex_s15"])
def test_probe_colours_equal_one_oracle_pass(rendered, name):
    fx, probe, _ = rendered[name]
    lp = np.zeros(oracle.LIGHT_POINTS, oracle.LIGHTPATH_DTYPE)
    col, cnt, _ = oracle.path_passes(fx["spheres"], fixture_table(fx), camera_of(fx), fx["W"], fx["H"], lp,
                                     [fx["sid"]], [1])
    assert (cnt == 1).all()
    same(probe_chain_colors(fx["spheres"], probe["pass"]), col.reshape(fx["H"], fx["W"], 3), name)


@pytest.mark.parametrize("name", [n for n in CASES if n.endswith("_const")])
def test_transmit_equals_pass_on_the_constant_table(rendered, name):
    fx, probe, own = rendered[name]
    assert fx["table"] == CONST
    same_chain(probe["transmit"], probe["pass"], f"{name} probe")
    same_chain(own["transmit"], own["pass"], name)


def test_the_branches_differ_where_the_pass_reflects(rendered):
    """The choice matters: on the seed-15 table some glass vertices reflect, on the zero table all
    with a choice do."""
    for name in ("mirror_s15", "glass_s15", "mirror_zero"):
        _, probe, _ = rendered[name]
        assert (bits(probe["transmit"]["throughput"]) != bits(probe["pass"]["throughput"])).any(), name


@pytest.mark.parametrize("name", CASES)
def test_first_hit_planes(rendered, name):
    """first_id is render_aov's id everywhere; where bounces == 0 the six shared planes are
    render_aov's; the kinds mean what the header says."""
    fx, _, own = rendered[name]
    with g.Renderer(fx["scene_spheres"], fx["W"], fx["H"], camera_of(fx), device=CPU) as r:
        set_table(r, fx)
        aov = r.render_aov(sid=fx["sid"])
    sp = fx["scene_spheres"]
    for branch in ("pass", "transmit"):
        c = own[branch]
        same(c["first_id"], aov["id"], f"{name} {branch}: first_id")
        z = c["bounces"] == 0
        for k in SHARED:
            same(c[k][z], aov[k][z], f"{name} {branch}: {k} where bounces == 0")
        ended = (c["kind"] == KIND_DIFFUSE) | (c["kind"] == KIND_EMITTER)
        assert np.array_equal(c["id"] >= 0, ended)
        assert (c["kind"][c["first_id"] < 0] == KIND_MISS).all() and (c["bounces"][c["kind"] == KIND_EXHAUSTED] == 7).all()
        emis = (sp["e"] != 0).any(axis=1)
        idx = np.where(ended, c["id"], 0)
        assert np.array_equal(emis[idx][ended], (c["kind"] == KIND_EMITTER)[ended])
        assert (sp["refl"][idx][c["kind"] == KIND_DIFFUSE] == g.DIFF).all()
        for k in ("dp", "position", "normal"):
            assert (bits(c[k][~ended]) == 0).all(), f"{name} {branch}: {k} is not +0 without an end vertex"
        assert (c["bounces"] >= 0).all() and (c["bounces"] <= 7).all()


def test_fixtures_cover_what_they_claim():
    """The committed meta file describes the committed fixtures: the statement's coverage counts per
    case are the recorded ones, and they meet what the fixtures are for."""
    assert CASES == [c["name"] for c in mrc.cases()]
    tir = 0
    for m in META["cases"]:
        fx = load_case(m["name"])
        assert m["size"] == [fx["W"], fx["H"]] and m["table"] == fx["table"] and m["spheres"] == len(fx["spheres"])
        assert os.path.getsize(os.path.join(GOLDEN, f"ref_chain_{m['name']}.npz")) <= 32768
        cov = coverage(statement_case(fx, fx["spheres"], "pass"))
        assert cov == m["coverage"], m["name"]
        mrc.check_coverage({"name": m["name"], "scene": m["scene"]}, cov)
        tir += cov["tir"]
    assert tir == META["tir_total"] > 0
    assert {tuple(m["size"]) for m in META["cases"]} == {(20, 19), (33, 9)}
    assert len(load_case("complex_s15")["spheres"]) == 783


@pytest.mark.skipif(not R.available(), reason="no reference build and no reference tree")
@pytest.mark.parametrize("name", CASES)
def test_fixture_regenerates(name):
    """Regenerating tests/golden/ref_chain_<name>.npz reproduces the committed bytes of every array."""
    lib = R.ref()
    case = {c["name"]: c for c in mrc.cases()}[name]
    fx = load_case(name)
    want = mrc.fixture_arrays(case, mrc.run_reference(case, lib, fixture_table(fx)))
    have = np.load(os.path.join(GOLDEN, f"ref_chain_{name}.npz"))
    assert sorted(have.files) == sorted(want)
    for k, v in want.items():
        v = np.asarray(v)
        assert v.dtype == have[k].dtype and v.tobytes() == have[k].tobytes(), f"ref_chain_{name}.npz[{k}]"


@pytest.mark.parametrize("sid", wrap_sids(20, 19)[:2] + [g.RAND_N - 1])
def test_sid_wrap_and_last_sid(sid):
    """j = (26 + 25 i + 5 depth + sid) mod (RAND_N - 5) wraps inside the frame; sid = RAND_N - 1."""
    cam, sp = scene("cornell_glass", 20, 19)
    with g.Renderer(sp, 20, 19, cam, device=CPU) as r:
        r.generate_rand(15)
        rnd = r.read_rand()
        for branch in ("pass", "transmit"):
            same_chain(r.render_chain(sid=sid, branch=branch), np_chain(sp, cam_floats(cam), 20, 19, rnd, sid, branch),
                       f"sid {sid} {branch}")


def test_unjittered_and_windows_equal_slices():
    cam, sp = scene("cornell_mirror", 20, 19)
    with g.Renderer(sp, 20, 19, cam, device=CPU) as r:
        whole0 = r.render_chain()
        same_chain(whole0, np_chain(sp, cam_floats(cam), 20, 19), "unjittered")
        r.generate_rand(15)
        whole = r.render_chain(sid=7, branch="pass")
        for x0, y0, w, h in [(7, 3, 13, 5), (3, 4, 1, 1), (19, 18, 1, 1), (0, 0, 20, 1), (19, 0, 1, 19)]:
            win = r.render_chain(sid=7, branch="pass", window=(x0, y0, w, h))
            win0 = r.render_chain(window=(x0, y0, w, h))
            for k in PLANES:
                same(win[k], whole[k][y0:y0 + h, x0:x0 + w], f"window {(x0, y0, w, h)} {k}")
                same(win0[k], whole0[k][y0:y0 + h, x0:x0 + w], f"unjittered window {(x0, y0, w, h)} {k}")


def test_errors():
    """(A multi-device context exists on GPUs only: tests/test_gpu_chain.py refuses it there.)"""
    assert_errors(CPU)


def test_passes_after_render_chain_equal_passes_without_it():
    assert_non_interference(CPU, "cornell_mirror", 33, 25)


def test_command_line_adds_the_chain_planes(tmp_path):
    """python -m gpu_bidirectional_raytracer_amd.aov --through: the .npz also holds the chain planes
    as chain_<plane>, --ppm also writes PREFIX_through_normal.ppm."""
    from gpu_bidirectional_raytracer_amd import aov as cli
    scn = os.path.join(g.SCENE_DIR, "cornell_mirror.scn")
    prefix = str(tmp_path / "m")
    assert cli.main(["19", "18", scn, "--out", prefix, "--device", "-1", "--ppm", "--through"]) == 0
    got = np.load(prefix + ".npz")
    cam, sp = scene("cornell_mirror", 20, 19)
    with g.Renderer(sp, 20, 19, cam, device=CPU) as r:
        want, aov = r.render_chain(), r.render_aov()
    assert sorted(got.files) == sorted(list(g.AOV_PLANES) + [f"chain_{k}" for k in PLANES])
    for k in PLANES:
        same(got[f"chain_{k}"], want[k], k)
    for k in g.AOV_PLANES:
        same(got[k], aov[k], k)
    assert open(tmp_path / "m_through_normal.ppm").read(20).split()[:4] == ["P3", "20", "19", "255"]
