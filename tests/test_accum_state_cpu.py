"""The scenarios of tests/accum_modes.py on the host (CPU) backend against the oracle, bit for bit:
an accumulation state that differs from pixel to pixel (counters at, below, across and above the
30000 cap), and shard changes and a reset between calls.  Also what `uneven_state` promises, so the
GPU tests of tests/test_gpu_accum_state.py stand on a checked builder.  Runs without a GPU."""
import numpy as np
import pytest

import oracle
import accum_modes as am

CPU = -1


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


def test_uneven_state_properties():
    col, cnt = am.uneven_state(am.W, am.H, 7)
    assert col.shape == (am.H, am.W, 3) and col.dtype == np.float32
    assert cnt.shape == (am.H, am.W) and cnt.dtype == np.uint32
    c = cnt.reshape(-1)
    assert int(c.max()) <= am.CAP + 1
    for v in am.CYCLE:
        assert (c == v).any(), f"no pixel starts at {v}"
    # runs of pixels at the cap: each longer than a wave (64), shorter than a pool chunk (128), and
    # followed by an uncapped pixel within 64 more
    at = c == am.CAP
    edges = np.flatnonzero(np.diff(np.concatenate(([0], at.astype(np.int8), [0]))))
    starts, ends = edges[::2], edges[1::2]
    assert len(starts) >= 40
    whole = ends < len(c)                                    # runs the frame's end does not cut
    assert ((ends - starts)[whole] >= 64).all() and ((ends - starts) < 128).all()
    for s, e in zip(starts[whole], ends[whole]):
        assert not at[e] and e - (s + 64) < 64
    # a run starts at every even residue mod 64, so whatever a chunk's alignment some chunk begins
    # with 64 capped pixels and goes on with uncapped ones
    assert set(int(s) % 64 for s in starts) == set(range(0, 64, 2))
    for chunk in (128, 256):
        heads = [q for q in range(0, len(c), chunk) if at[q:q + 64].all() and len(at[q:q + 64]) == 64]
        assert any((c[q + 64:q + chunk] < am.CAP).any() for q in heads), chunk
    # colours: float32 in [0, 4), a few exact zeros on capped and uncapped pixels, channels differ
    assert (col >= 0).all() and (col < 4).all()
    zero = (col == 0).any(-1)
    assert 20 <= int(zero.sum()) <= 400 and (zero & (cnt >= am.CAP)).any() and (zero & (cnt < am.CAP)).any()
    assert (col[..., 0] != col[..., 1]).mean() > 0.95 and (col[..., 1] != col[..., 2]).mean() > 0.95
    col2, cnt2 = am.uneven_state(am.W, am.H, 7)
    assert col.tobytes() == col2.tobytes() and cnt.tobytes() == cnt2.tobytes()


def test_closed_form_counter():
    c0 = np.array([0, 29979, 29985, 29999, 30000, 30001], np.uint32)
    assert am.closed_form_counter(c0, 20).tolist() == [20, 29999, 30000, 30000, 30000, 30001]


def test_launch_passes():
    """How bdpt_path_passes cuts a call (bdpt_host.cpp one_path_passes: equal launches)."""
    assert am.launch_passes(20, 6, False) == (5, 4)
    assert am.launch_passes(36, 12, False) == (12, 3)
    assert am.launch_passes(9, None, False) == (9, 1)
    assert am.launch_passes(200, None, False) == (100, 2)
    assert am.launch_passes(100, None, True) == (50, 2)


@pytest.mark.parametrize("scene", ["cornell", "caustic", "synthetic64"])
def test_uneven_state_cpu(scene):
    sc = am.uneven(scene)
    got = am.run(None, sc, CPU)
    col0, cnt0 = am.uneven_state(am.W, am.H, 7)
    am.same(got[0][0], col0, "colours read back")
    am.same(got[0][1], cnt0, "counters read back")
    to_int = np.vectorize(oracle.to_int, otypes=[np.uint8])   # write_radiance: pixel = toInt(colour)
    am.same(got[0][2][..., :3], to_int(col0), "pixels after write_radiance")
    am.check(sc, got, f"cpu {scene}")


def test_state_changes_between_calls_cpu():
    sc = am.state_changes()
    got = am.run(None, sc, CPU)
    am.check(sc, got, "cpu")
    # counters by band after the second call: 12 on the rows shard 1 of 3 owned, 7 elsewhere
    owned = (np.arange(am.H) // 8) % 3 == 1
    assert (got[2][1][owned] == 12).all() and (got[2][1][~owned] == 7).all()
    assert (got[3][1] == 4).all()
