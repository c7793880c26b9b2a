"""Every kernel mode of the path integrator (tests/accum_modes.py: fused with paired and unpaired
loads, two, four and one pass(es) per lane, a fixed S, pixel pools, the ordered in-kernel fold, the
precompiled builds and the BVH build) on the inputs the fresh-frame tests do not give them:

- an accumulation state that is not uniform over the frame (bdpt_write_radiance: "rendering then
  continues from that state bit for bit"): runs of pixels at the 30000 cap longer than a wave and
  shorter than a pool chunk, next to pixels at 0, young ones, ones that cross the cap in the first
  or the second call, and one above it;
- calls cut into four launches (three for four passes per lane) with BDPT_MAX_LAUNCH_PASSES: the
  third launch is the first that reuses a half of the radiance buffer, a pool-counter set or a
  flag array of the units and has to wait for an earlier fold;
- both together, so the cap falls in a launch whose predecessor's fold may still be pending;
- a shard change (which grows the units' flag array) and a reset between calls.

Frames are 97 x 65 (both packed edges), at most 36 passes.  Every comparison is bit for bit against
the oracle chained call by call, colours as uint32 with counters and pixels, and every case proves
the mode it asked for ran (last_streams, last_features, last_specialized, stream_choice, the
launch count)."""
import pytest

import accum_modes as am

pytestmark = pytest.mark.gpu

SPARSE = ("pool2", "pool4", "units3")           # also on caustic: most of its samples are +0


def _scene(mode):
    return "synthetic64" if mode.bvh else "cornell"


def _case(mode, sc, gpu, monkeypatch):
    am.check(sc, am.run(mode, sc, gpu, monkeypatch), f"{mode.name} {sc.scene} {sc.name}")


@pytest.mark.parametrize("name,scene", [(m.name, _scene(m)) for m in am.MODES] + [(n, "caustic") for n in SPARSE])
def test_uneven_state_every_mode(gpu, name, scene, monkeypatch):
    _case(am.BY_NAME[name], am.uneven(scene), gpu, monkeypatch)


@pytest.mark.parametrize("name", [m.name for m in am.MODES])
def test_split_calls_every_mode(gpu, name, monkeypatch):
    mode = am.BY_NAME[name]
    # 20 passes in 4 launches of 5; four per lane needs launches of >= 8: 36 in 3 of 12 (S = 3)
    sc = am.split(36, 12, _scene(mode)) if name == "four_per_lane" else am.split(20, 6, _scene(mode))
    _case(mode, sc, gpu, monkeypatch)


@pytest.mark.parametrize("name", ["two_per_lane", "one_per_lane", "pool4", "units3"])
def test_uneven_state_split_calls(gpu, name, monkeypatch):
    _case(am.BY_NAME[name], am.uneven_split(), gpu, monkeypatch)


@pytest.mark.parametrize("name", ["units3", "pool4", "two_per_lane"])
def test_state_changes_between_calls(gpu, name, monkeypatch):
    _case(am.BY_NAME[name], am.state_changes(), gpu, monkeypatch)
