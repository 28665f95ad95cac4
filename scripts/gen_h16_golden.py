#!/usr/bin/env python3
"""Writes tests/golden/cdf97_h.npz and tests/golden/cdf97_h_manifest.json: the float CDF 9/7 on binary16 storage
(DWT_HIP_CDF97_H; tests/f16_model.py) computed with the COMPILED REFERENCE -- per level the reference's
dwt_cdf97_2f_s / dwt_cdf97_2i_s at one level on the level's frame in binary32, followed by numpy's rounding to binary16.

Per case the file holds the input, the forward result and the inverse of that result, as 16-bit patterns.  The generator
ASSERTS on every case that the reference's chain equals tests/f16_model.py (the same chain on the oracle restatement), and
that the chain without the rounding equals the reference's own multi-level transform bit for bit, and fails otherwise.

The reference is oraclelib.Reference: oracle/_ref/libdwt_ref.so, built from the reference's sources where they lie by the
recipe of oracle/Makefile; nothing of it enters the tree.

    python scripts/gen_h16_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f16_model as M  # noqa: E402
import oraclelib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "cdf97_h.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "cdf97_h_manifest.json")

SHAPES = [(2, 2), (3, 5), (9, 14), (13, 7), (32, 32), (67, 130)]  # (rows, columns)
LEVELS = [1, 2, -1]
# (rows, columns) of the outer frame, (rows, columns) of the inner one, j_max, decompose_one, zero_padding
SPECIAL = [((40, 50), (29, 37), 3, 0, 0), ((40, 50), (29, 37), 3, 0, 1), ((5, 70), (5, 70), -1, 1, 0)]


def same16(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb])


def main():
    ref = oraclelib.Reference()
    rng = np.random.default_rng(9716)
    out, cases = {}, []

    def add(shape, inner, j_max, decompose_one, zero_padding, kind):
        i = len(cases)
        x = (rng.integers(0, 256, size=shape) if kind == "8bit" else rng.random(shape, dtype=np.float32)).astype(np.float16)
        so, si = (shape[1], shape[0]), (inner[1], inner[0])
        kw = dict(size_o=so, size_i=si, decompose_one=decompose_one, zero_padding=zero_padding)
        M.assert_chain_is_multilevel(x.astype(np.float32), j_max=j_max, lib=ref, **kw)
        M.assert_chain_is_multilevel(x.astype(np.float32), j_max=j_max, **kw)
        f_ref, f_mod = x.copy(), x.copy()
        j = M.fwd2d(f_ref, j_max=j_max, lib=ref, **kw)
        assert M.fwd2d(f_mod, j_max=j_max, **kw) == j and same16(f_ref, f_mod), ("reference != model", "forward", shape, j_max)
        b_ref, b_mod = f_ref.copy(), f_ref.copy()
        M.inv2d(b_ref, j_max=j, lib=ref, **kw)
        M.inv2d(b_mod, j_max=j, **kw)
        assert same16(b_ref, b_mod), ("reference != model", "inverse", shape, j_max)
        out["in_%d" % i], out["fwd_%d" % i], out["inv_%d" % i] = x.view(np.uint16), f_ref.view(np.uint16), b_ref.view(np.uint16)
        cases.append({"size_o": list(so), "size_i": list(si), "j_max": j_max, "levels": j, "decompose_one": decompose_one,
                      "zero_padding": zero_padding, "input": kind})

    for shape in SHAPES:
        for j_max in LEVELS:
            for kind in ("8bit", "unit"):
                add(shape, shape, j_max, 0, 0, kind)
    for shape, inner, j_max, d1, zp in SPECIAL:
        add(shape, inner, j_max, d1, zp, "8bit")

    np.savez_compressed(GOLDEN, **out)
    with open(GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_h16_golden.py",
                   "reference": "libdwt (dwt_cdf97_2f_s / dwt_cdf97_2i_s at one level per level, numpy astype(float16) after each; oracle/Makefile ref)",
                   "asserted": "reference chain == tests/f16_model.py on every case; unrounded chain == the reference's multi-level transform",
                   "layout": "in_i / fwd_i / inv_i: uint16 patterns of binary16 samples, rows = y; size_o / size_i as (x, y)",
                   "files": {"cdf97_h.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
