#!/usr/bin/env python3
"""Writes tests/golden/swt2d.npz and tests/golden/swt2d_manifest.json: the reference's swt_cdf97_f_ex_stride_s /
swt_cdf53_f_ex_stride_s run over the rows (stride 4) and then over the columns (stride = pitch) of the images of
tests/swt2d_model.py, level after level on the LL plane.  Per case the detail planes of every level (HL, LH, HH) and the
last level's LL are stored.

The reference's swt.c, util.c, signal.c, libdwt.c and system.c are compiled from where they lie with the reference's own
release flags (oracle/Makefile: REF_CFLAGS) into a temporary directory outside the repository, loaded from there, and the
directory is deleted: no reference text or binary enters the tree.

    python scripts/gen_swt2d_golden.py [--ref /path/to/libdwt]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import swt2d_model as m2  # noqa: E402
from gen_swt_golden import REF_SRCS, ref_cflags  # noqa: E402


def level(fn, a, l):
    """(LL, HL, LH, HH) of image a: the reference's function along every row, then along every column"""
    h, w = a.shape
    a = np.ascontiguousarray(a, np.float32)
    lr, hr = np.zeros_like(a), np.zeros_like(a)
    for y in range(h):
        fn(a[y].ctypes.data, lr[y].ctypes.data, hr[y].ctypes.data, w, 4, l)
    out = [np.zeros_like(a) for _ in range(4)]  # LL, LH (from Lr), HL, HH (from Hr)
    for x in range(w):
        fn(lr.ctypes.data + 4 * x, out[0].ctypes.data + 4 * x, out[1].ctypes.data + 4 * x, h, 4 * w, l)
        fn(hr.ctypes.data + 4 * x, out[2].ctypes.data + 4 * x, out[3].ctypes.data + 4 * x, h, 4 * w, l)
    return out[0], out[2], out[1], out[3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    tmp = tempfile.mkdtemp(prefix="swt2d_golden_")
    try:
        so = os.path.join(tmp, "libswt_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        out, cases = {}, []
        for i, (seed, wavelet, kind, size_y, size_x, levels) in enumerate(m2.CASES):
            fn = getattr(lib, {"cdf97_s": "swt_cdf97_f_ex_stride_s", "cdf53_s": "swt_cdf53_f_ex_stride_s"}[wavelet])
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
            fn.restype = None
            cur = m2.make_input(seed, kind, size_y, size_x)
            D = np.zeros((levels, 3, size_y, size_x), np.float32)
            for l in range(levels):
                cur, D[l, 0], D[l, 1], D[l, 2] = level(fn, cur, l)
            out["D_%d" % i], out["LL_%d" % i] = D, cur
            cases.append({"seed": seed, "wavelet": wavelet, "kind": kind, "size_y": size_y, "size_x": size_x, "levels": levels})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(m2.GOLDEN, **out)
    with open(m2.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(m2.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_swt2d_golden.py", "reference": "libdwt (src/swt.c, src/util.c, src/signal.c; oracle/Makefile REF_CFLAGS)",
                   "files": {"swt2d.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", m2.GOLDEN, os.path.getsize(m2.GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
