"""tests/golden/make_golden_minrep.py -- golden_minrep.npz: polyhedra {x : A x <= b} and the REFERENCE's daqp_minrep verdicts
(strict-IEEE build, oracle/_ref: build container only; CPU only).

Generator, per polyhedron of shape (n, m, ms):
  * max(n + 1, (m - ms) // 2) unit rows with b in [1, 1.3];
  * the remaining general rows are non-negative combinations of three of those rows, their right-hand side the same combination
    of the three b pushed out by [0.05, 0.5] * |row| -- redundant by construction, with a clear margin;
  * rows rescaled by [0.5, 2] and permuted; simple bounds, if any, x_i <= b_i with b_i in [0.3, 3];
  * A and b are rounded to fp32 values (the fixture stores four bytes per entry; the reference and the GPU both get exactly these).

Inclusion condition (a polyhedron is kept only if both hold; at most one in ten may be dropped):
  * the reference's verdicts do not change when every b_i is pushed by a relative 1e-4 towards the other verdict;
  * they do not change when the rows are normalised to unit length first (the GPU path normalises: primal_tol is compared with the
    normalised slack there and with the raw slack in the reference -- this keeps every margin clear of that difference).

Stored per shape key "n_m_ms": A (4, m - ms, n) float32, b (4, m) float32, red (4, m) int8.  Data only.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(3, 12, 0), (8, 64, 0), (8, 65, 0), (6, 40, 6), (12, 130, 0), (50, 150, 0), (64, 256, 0), (80, 200, 0)]
PER_SHAPE = 4
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def generate(n, m, ms, seed):
    """one polyhedron: A (m - ms, n) and b (m,), fp32-representable doubles"""
    rng = np.random.default_rng([2026, n, m, ms, seed])
    mA = m - ms
    nu = min(mA, max(n + 1, mA // 2))
    U = rng.standard_normal((nu, n))
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    bU = rng.uniform(1.0, 1.3, nu)
    rows, rhs = [U], [bU]
    for _ in range(mA - nu):
        k = rng.choice(nu, 3, replace=False)
        c = rng.uniform(0.2, 1.0, 3)
        r = c @ U[k]
        rows.append(r[None, :])
        rhs.append(np.array([c @ bU[k] + rng.uniform(0.05, 0.5) * np.linalg.norm(r)]))
    A, bA = np.vstack(rows), np.concatenate(rhs)
    s = rng.uniform(0.5, 2.0, mA)
    perm = rng.permutation(mA)
    A, bA = (A * s[:, None])[perm], (bA * s)[perm]
    b = np.concatenate([rng.uniform(0.3, 3.0, ms), bA])
    return A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)


class RefMinrep:
    def __init__(self):
        O.build()
        self.lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libdaqp_ref_strict.so"))
        self.lib.daqp_minrep.argtypes = [_ip, _dp, _dp, C.c_int, C.c_int, C.c_int]
        self.lib.daqp_minrep.restype = None

    def __call__(self, A, b, ms):
        A, b = np.ascontiguousarray(A, np.float64).copy(), np.ascontiguousarray(b, np.float64).copy()
        m, n = b.size, A.shape[1]
        out = np.full(m, -7, np.int32)
        self.lib.daqp_minrep(out.ctypes.data_as(_ip), A.ctypes.data_as(_dp), b.ctypes.data_as(_dp), n, m, ms)
        return out


def stable(ref, A, b, ms, red):
    """the inclusion condition"""
    push = np.where(red == 1, -1.0, 1.0) * 1e-4 * np.abs(b)
    if not np.array_equal(ref(A, b + push, ms), red):
        return False
    nrm = np.linalg.norm(A, axis=1)
    bn = b.copy()
    bn[ms:] = b[ms:] / nrm
    return np.array_equal(ref(A / nrm[:, None], bn, ms), red)


def entry(ref, n, m, ms, k):
    """the k-th kept polyhedron of a shape and how many candidates were dropped before it"""
    kept, dropped, seed = 0, 0, 0
    while True:
        A, b = generate(n, m, ms, seed)
        seed += 1
        red = ref(A, b, ms)
        if set(np.unique(red)) <= {0, 1} and stable(ref, A, b, ms, red):
            if kept == k:
                return A, b, red, dropped
            kept += 1
        else:
            dropped += 1


def main():
    ref = RefMinrep()
    out, tried, dropped_all = {}, 0, 0
    for n, m, ms in SHAPES:
        As, bs, reds = [], [], []
        for k in range(PER_SHAPE):
            A, b, red, dropped = entry(ref, n, m, ms, k)
            As.append(A), bs.append(b), reds.append(red)
        tried += PER_SHAPE + dropped
        dropped_all += dropped
        key = f"{n}_{m}_{ms}"
        out["A_" + key] = np.stack(As).astype(np.float32)
        out["b_" + key] = np.stack(bs).astype(np.float32)
        out["red_" + key] = np.stack(reds).astype(np.int8)
        frac = np.stack(reds).mean(axis=1)
        print(f"{key}: redundant fraction per polyhedron {np.round(frac, 2)}, candidates dropped {dropped}")
    assert dropped_all * 10 <= tried, f"the inclusion condition dropped {dropped_all} of {tried} candidates"
    path = os.path.join(HERE, "golden_minrep.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
