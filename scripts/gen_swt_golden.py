#!/usr/bin/env python3
"""Writes tests/golden/swt.npz and tests/golden/swt_manifest.json: the outputs of the reference's
swt_cdf97_f_ex_stride_s / swt_cdf53_f_ex_stride_s for the cases of tests/swt_model.py.

The reference's swt.c, util.c and signal.c (and libdwt.c, which util.c links against) are compiled from where they lie
with the reference's own release flags (oracle/Makefile: REF_CFLAGS) into a temporary directory outside the repository,
loaded from there, and the directory is deleted: no reference text or binary enters the tree.

    python scripts/gen_swt_golden.py [--ref /path/to/libdwt]
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
import swt_model as sm  # noqa: E402

REF_SRCS = ["swt.c", "util.c", "signal.c", "libdwt.c", "system.c"]


def ref_cflags(ref):
    version = open(os.path.join(ref, "VERSION")).read().strip() if os.path.exists(os.path.join(ref, "VERSION")) else ""
    return ["-std=c99", "-O3", "-ftree-vectorize", "-fopenmp", "-fPIC", "-finline-functions", "-DNDEBUG",
            "-D_POSIX_C_SOURCE=199309L", "-D_GNU_SOURCE", '-DPACKAGE_VERSION="%s"' % version, '-DPACKAGE_NAME="libdwt"',
            '-DPACKAGE_STRING="libdwt %s"' % version, '-DARCH="x86_64"', "-w"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    tmp = tempfile.mkdtemp(prefix="swt_golden_")
    try:
        so = os.path.join(tmp, "libswt_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        out, cases = {}, []
        for i, (seed, wavelet, kind, n, levels) in enumerate(sm.CASES):
            fn = getattr(lib, {"cdf97_s": "swt_cdf97_f_ex_stride_s", "cdf53_s": "swt_cdf53_f_ex_stride_s"}[wavelet])
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
            fn.restype = None
            x = np.ascontiguousarray(sm.make_input(seed, kind, 1, n)[0])
            L = np.zeros((levels, n), np.float32)
            H = np.zeros((levels, n), np.float32)
            cur = x
            for l in range(levels):
                fn(cur.ctypes.data, L[l].ctypes.data, H[l].ctypes.data, n, 4, l)
                cur = L[l]
            out["L_%d" % i], out["H_%d" % i] = L, H
            cases.append({"seed": seed, "wavelet": wavelet, "kind": kind, "n": n, "levels": levels})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(sm.GOLDEN, **out)
    with open(sm.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(sm.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_swt_golden.py", "reference": "libdwt (src/swt.c, src/util.c, src/signal.c; oracle/Makefile REF_CFLAGS)",
                   "files": {"swt.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", sm.GOLDEN, os.path.getsize(sm.GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
