"""Writes tests/golden/interp53.npz: inputs and results of libdwt's own dwt_interp53_2f_s / _2i_s / _1f_s / _1i_s
(oracle/_ref/libdwt_ref.so, built by `make -C oracle ref`), for tests/test_interp53.py on machines where the reference
is not built.  Each case stores its input, the forward result and the inverse of that result.

    python scripts/gen_interp53_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import interp53_model as M  # noqa: E402
from conftest import full_range_floats  # noqa: E402

# 2-D: (shape, size_i or None, j_max, decompose_one, zero_padding, whole float range)
CASES_2D = []
for shape in [(1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (9, 14), (16, 7)]:
    for j_max, d1 in [(-1, 0), (-1, 1), (0, 0), (2, 1), (40, 0)]:
        CASES_2D.append((shape, None, j_max, d1, 0, False))
for zp in (0, 1):
    for d1 in (0, 1):
        CASES_2D.append(((40, 50), (29, 37), 3, d1, zp, False))
        CASES_2D.append(((1, 33), (1, 20), -1, d1, zp, False))
CASES_2D.append(((37, 100), None, -1, 0, 0, False))
CASES_2D.append(((67, 130), None, -1, 0, 0, True))
# 1-D: (n_lines, size_o, size_i or None, j_max, zero_padding, whole float range)
CASES_1D = []
for so in (1, 2, 3, 5, 8, 37, 64):
    for j_max in (-1, 0, 2, 40):
        CASES_1D.append((3, so, None, j_max, 0, False))
for zp in (0, 1):
    CASES_1D.append((2, 50, 29, 3, zp, False))
    CASES_1D.append((2, 33, 1, -1, zp, False))
    CASES_1D.append((1, 1, 0, -1, zp, False))
CASES_1D.append((4, 1000, None, -1, 0, True))


def main():
    ref = M.RefInterp53()
    rng = np.random.default_rng(53)
    out = {}
    for n, (shape, si, j_max, d1, zp, full) in enumerate(CASES_2D):
        img = full_range_floats(rng, shape, klass="mixed", nonfinite=True) if full else (rng.random(shape, dtype=np.float32) * 8 - 4)
        a = img.copy()
        j = ref.fwd2d(a, size_i=si, j_max=j_max, decompose_one=d1, zero_padding=zp)
        b = a.copy()
        ref.inv2d(b, size_i=si, j_max=j, decompose_one=d1, zero_padding=zp)
        out["t%d_meta" % n] = np.array([-1 if si is None else si[0], -1 if si is None else si[1], j_max, d1, zp, j], dtype=np.int32)
        out["t%d_in" % n], out["t%d_fwd" % n], out["t%d_inv" % n] = img, a, b
    for n, (lines, so, si, j_max, zp, full) in enumerate(CASES_1D):
        x = full_range_floats(rng, (lines, so), klass="mixed", nonfinite=True) if full else (rng.random((lines, so), dtype=np.float32) * 8 - 4)
        a = x.copy()
        j = ref.fwd1d(a, size_i=si, j_max=j_max, zero_padding=zp)
        b = a.copy()
        ref.inv1d(b, size_i=si, j_max=j, zero_padding=zp)
        out["o%d_meta" % n] = np.array([-1 if si is None else si, j_max, zp, j], dtype=np.int32)
        out["o%d_in" % n], out["o%d_fwd" % n], out["o%d_inv" % n] = x, a, b
    path = os.path.join(ROOT, "tests", "golden", "interp53.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES_2D), "2-D and", len(CASES_1D), "1-D cases")


if __name__ == "__main__":
    main()
