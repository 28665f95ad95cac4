#!/usr/bin/env python3
"""Writes tests/golden/eaw97.npz and tests/golden/eaw97_manifest.json: inputs, coefficients, every wH[k] / wV[k] and the
inverse's output of the reference's dwt_eaw97_2f_s / dwt_eaw97_2i_s for the cases of tests/eaw97_model.py.  Weight
entries the reference leaves unwritten (one-sample lines) are stored as NaN, as in eaw53.npz.

The reference's eaw-experimental.c, libdwt.c and system.c are compiled from where they lie with the reference's own
release flags (oracle/Makefile: REF_CFLAGS) into a temporary directory outside the repository, loaded from there, and
the directory is deleted: no reference text or binary enters the tree.

The manifest also records two tolerances measured from these fixtures (tests/test_eaw97.py recomputes them):
alpha_dev_model, the largest deviation of the model's coefficients with pow-in-double weights from the reference's at
alpha 0.8, relative to the largest coefficient; and roundtrip_ref, the reference's own round-trip error relative to
max|input| over the dense cases with inputs in [-4, 4).

    python scripts/gen_eaw97_golden.py [--ref /path/to/libdwt]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eaw97_model as M  # noqa: E402
from conftest import full_range_floats  # noqa: E402

REF_SRCS = ["eaw-experimental.c", "libdwt.c", "system.c"]


def ref_cflags(ref):
    version = open(os.path.join(ref, "VERSION")).read().strip() if os.path.exists(os.path.join(ref, "VERSION")) else ""
    return ["-std=c99", "-O3", "-ftree-vectorize", "-fopenmp", "-fPIC", "-finline-functions", "-DNDEBUG",
            "-D_POSIX_C_SOURCE=199309L", "-D_GNU_SOURCE", '-DPACKAGE_VERSION="%s"' % version, '-DPACKAGE_NAME="libdwt"',
            '-DPACKAGE_STRING="libdwt %s"' % version, '-DARCH="x86_64"', "-w"]


def run_case(lib, libc, img, si, j_max, d1, zp, alpha):
    """(coefficients, j, wH, wV, inverse of the coefficients) of the reference on a copy of img."""
    soy, sox = img.shape
    siy, six = si or (soy, sox)
    a = img.copy()
    hp, vp = (C.c_void_p * 64)(), (C.c_void_p * 64)()
    j = C.c_int(j_max)
    lib.dwt_eaw97_2f_s(a.ctypes.data, a.strides[0], 4, sox, soy, six, siy, C.byref(j), d1, zp, C.cast(hp, C.c_void_p),
                       C.cast(vp, C.c_void_p), alpha)
    back = a.copy()
    lib.dwt_eaw97_2i_s(back.ctypes.data, back.strides[0], 4, sox, soy, six, siy, j.value, d1, zp, C.cast(hp, C.c_void_p),
                       C.cast(vp, C.c_void_p))
    wH, wV = [], []
    for k in range(j.value):
        Hi, Wi = M.ceil_div_pow2(siy, k), M.ceil_div_pow2(six, k)
        for p, shape, out in ((hp[k], (M.ceil_div_pow2(soy, k), Wi), wH), (vp[k], (M.ceil_div_pow2(sox, k), Hi), wV)):
            n = shape[0] * shape[1]
            w = np.ctypeslib.as_array((C.c_float * n).from_address(p)).reshape(shape).copy() if n else np.zeros(shape, np.float32)
            if shape[1] == 1:
                w[:] = np.nan  # uninitialised in the reference
            out.append(w)
            libc.free(p)
    return a, j.value, wH, wV, back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    tmp = tempfile.mkdtemp(prefix="eaw97_golden_")
    out, cases = {}, []
    try:
        so = os.path.join(tmp, "libeaw97_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        P, I = C.c_void_p, C.c_int
        lib.dwt_eaw97_2f_s.argtypes = [P, I, I, I, I, I, I, C.POINTER(I), I, I, P, P, C.c_float]
        lib.dwt_eaw97_2f_s.restype = None
        lib.dwt_eaw97_2i_s.argtypes = [P, I, I, I, I, I, I, I, I, I, P, P]
        lib.dwt_eaw97_2i_s.restype = None
        rng = np.random.default_rng(2097)
        for n, (shape, si, j_max, d1, zp, alpha, kind) in enumerate(M.CASES):
            if kind == "mixed":
                img = full_range_floats(rng, shape, klass="mixed")
            else:
                img = (rng.random(shape, dtype=np.float32) * 8 - 4).astype(np.float32)
            with np.errstate(all="ignore"):
                a, j, wH, wV, back = run_case(lib, libc, img, si, j_max, d1, zp, alpha)
            out["c%d_meta" % n] = np.array([shape[0], shape[1], -1 if si is None else si[0], -1 if si is None else si[1],
                                            j_max, d1, zp, M.KINDS.index(kind), j], dtype=np.int32)
            out["c%d_alpha" % n] = np.float32(alpha)
            out["c%d_in" % n], out["c%d_out" % n], out["c%d_back" % n] = img, a, back
            for k in range(j):
                out["c%d_wH%d" % (n, k)], out["c%d_wV%d" % (n, k)] = wH[k], wV[k]
            cases.append({"shape": list(shape), "size_i": None if si is None else list(si), "j_max": j_max, "decompose_one": d1,
                          "zero_padding": zp, "alpha": alpha, "input": kind, "levels": j})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(M.GOLDEN, **out)
    with open(M.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    loaded = M.load_golden()
    with open(M.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_eaw97_golden.py",
                   "reference": "libdwt (src/eaw-experimental.c, src/libdwt.c, src/system.c; oracle/Makefile REF_CFLAGS)",
                   "alpha_dev_model": M.alpha_deviation(loaded), "roundtrip_ref": M.roundtrip_deviation(loaded),
                   "files": {"eaw97.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", M.GOLDEN, os.path.getsize(M.GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
