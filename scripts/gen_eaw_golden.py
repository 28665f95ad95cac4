"""Writes tests/golden/eaw53.npz: inputs, coefficients and weights of libdwt's own dwt_eaw53_2f_s /
dwt_eaw53_2f_inplace_s (oracle/_ref/libdwt_ref.so, built by `make -C oracle ref`) at alpha 1 and 0, for
tests/test_eaw.py on machines where the reference is not built.  Weight entries the reference leaves unwritten
(one-sample lines) are stored as NaN.

    python scripts/gen_eaw_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eaw_model as M  # noqa: E402

# (name, shape, size_i or None, j_max, decompose_one, zero_padding, alpha, interleaved)
CASES = []
for shape in [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (9, 14)]:
    for j_max, d1 in [(-1, 0), (-1, 1), (0, 0), (1, 0), (3, 1), (40, 0)]:
        for il in (False, True):
            CASES.append((shape, None, j_max, d1, 0, 1.0, il))
for shape in [(37, 100), (61, 67)]:
    for il in (False, True):
        CASES.append((shape, None, -1, 0, 0, 1.0, il))
for shape in [(3, 5), (37, 100)]:
    CASES.append((shape, None, -1, 0, 0, 0.0, False))
for zp in (0, 1):
    for il in (False, True):
        CASES.append(((40, 50), (29, 37), 3, 0, zp, 1.0, il))


def main():
    ref = M.RefEaw()
    rng = np.random.default_rng(2015)
    out = {}
    for n, (shape, si, j_max, d1, zp, alpha, il) in enumerate(CASES):
        img = (rng.random(shape, dtype=np.float32) * 8 - 4).astype(np.float32)
        a = img.copy()
        j, wH, wV = ref.fwd(a, size_i=si, j_max=j_max, decompose_one=d1, zero_padding=zp, alpha=alpha, interleaved=il)
        out["c%d_meta" % n] = np.array([shape[0], shape[1], -1 if si is None else si[0], -1 if si is None else si[1],
                                        j_max, d1, zp, int(il), j], dtype=np.int32)
        out["c%d_alpha" % n] = np.float32(alpha)
        out["c%d_in" % n] = img
        out["c%d_out" % n] = a
        for k in range(j):
            out["c%d_wH%d" % (n, k)] = wH[k]
            out["c%d_wV%d" % (n, k)] = wV[k]
    path = os.path.join(ROOT, "tests", "golden", "eaw53.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
