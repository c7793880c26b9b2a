"""NumPy float32 restatement of the sample records (csrc/bdpt_math.h bdpt_sample_record), shared by
tests/test_sample_records.py and tests/test_gpu_sample_records.py: for table positions j the 8
floats {A, B, C, u2, X, Y, Z, u0} of u0..u4 = table[j..j+4], every operation one float32 operation
in the order of the path kernel's cosine_tail_sc / uniform_sphere_sc, with sinf / cosf evaluated
as float32(f(float64(x))) (the project's contract for them)."""
import numpy as np

F = np.float32


def records(table: np.ndarray, pos: np.ndarray) -> np.ndarray:
    table = np.ascontiguousarray(table, F)
    pos = np.asarray(pos, np.int64)
    u0, u1, u2, u3, u4 = (table[pos + k] for k in range(5))
    two_pi = F(2.0) * F(3.14159265358979323846)
    x0, x4 = two_pi * u0, two_pi * u4
    s0, c0 = np.sin(x0.astype(np.float64)).astype(F), np.cos(x0.astype(np.float64)).astype(F)
    s4, c4 = np.sin(x4.astype(np.float64)).astype(F), np.cos(x4.astype(np.float64)).astype(F)
    r2s = np.sqrt(u1)
    zz = F(1.0) - F(2.0) * u3
    q = F(1.0) - zz * zz
    r = np.sqrt(np.where(F(0.0) > q, F(0.0), q))
    out = np.empty((len(pos), 8), F)
    out[:, 0] = c0 * r2s
    out[:, 1] = s0 * r2s
    out[:, 2] = np.sqrt(F(1.0) - u1)
    out[:, 3] = u2
    out[:, 4] = r * c4
    out[:, 5] = r * s4
    out[:, 6] = zz
    out[:, 7] = u0
    assert out.dtype == F and x0.dtype == F and q.dtype == F
    return out
