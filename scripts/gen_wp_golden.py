#!/usr/bin/env python3
"""Writes tests/golden/wp.npz and tests/golden/wp_manifest.json: wavelet packets of the inputs of tests/wp_model.py, each
node of each level through the COMPILED REFERENCE -- in 1-D its one-level line functions dwt_cdf97_f_ex_stride_s /
dwt_cdf97_i_ex_stride_s and their 5/3 and interpolating 5/3 siblings, in 2-D one level of dwt_cdf97_2f_s / _2i_s and their
siblings on the node's rectangle.  Per case the forward packets of the seeded input (F_*) and the inverse packets of the
same input taken as leaves (I_*) are stored.

The reference's sources are compiled from where they lie with the reference's own release flags into a temporary directory
outside the repository, loaded from there, and the directory is deleted: no reference text or binary enters the tree.

    python scripts/gen_wp_golden.py [--ref /path/to/libdwt]
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
import wp_model as wp  # noqa: E402
from gen_swt_golden import REF_SRCS, ref_cflags  # noqa: E402

P, I = C.c_void_p, C.c_int


def lines(lib, wavelet, a, levels, inverse):
    """packets of every row of a, node by node through the reference's line functions (out of place into a copy)"""
    name = "dwt_%s_%s_ex_stride_s" % (wavelet[:-2], "i" if inverse else "f")
    fn = getattr(lib, name)
    fn.argtypes = [P, P, P, P, I, I]
    fn.restype = None
    cur = np.ascontiguousarray(a, np.float32).copy()
    N = cur.shape[1]
    tmp = np.zeros(N + 16, np.float32)
    for lev in (range(levels - 1, -1, -1) if inverse else range(levels)):
        nxt = cur.copy()
        for s, n in wp.nodes_recursive(N, lev):
            nl = (n + 1) // 2
            for y in range(cur.shape[0]):
                c, d = cur[y].ctypes.data + 4 * s, nxt[y].ctypes.data + 4 * s
                if inverse:
                    fn(c, c + 4 * nl, d, tmp.ctypes.data, n, 4)
                else:
                    fn(c, d, d + 4 * nl, tmp.ctypes.data, n, 4)
        cur = nxt
    return cur


def image(lib, wavelet, a, levels, inverse):
    """packets of the image a, one level of the reference's 2-D driver per node, in place on the node's rectangle"""
    fn = getattr(lib, "dwt_%s_2%s_s" % (wavelet[:-2], "i" if inverse else "f"))
    fn.argtypes = [P, I, I, I, I, I, I, I if inverse else C.POINTER(I), I, I]
    fn.restype = None
    cur = np.ascontiguousarray(a, np.float32).copy()
    size_y, size_x = cur.shape
    for lev in (range(levels - 1, -1, -1) if inverse else range(levels)):
        for sy, h in wp.nodes_recursive(size_y, lev):
            for sx, w in wp.nodes_recursive(size_x, lev):
                p = cur.ctypes.data + cur.strides[0] * sy + 4 * sx
                if inverse:
                    fn(p, cur.strides[0], 4, w, h, w, h, 1, 0, 0)
                else:
                    j = I(1)
                    fn(p, cur.strides[0], 4, w, h, w, h, C.byref(j), 0, 0)
                    assert j.value == 1
    return cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    tmp = tempfile.mkdtemp(prefix="wp_golden_")
    try:
        so = os.path.join(tmp, "libwp_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        out, cases = {}, []
        for i, (seed, wavelet, kind, n_lines, N, levels) in enumerate(wp.CASES_1D):
            x = wp.make_input(seed, kind, n_lines, N)
            out["F_" + wp.case_key(1, i)] = lines(lib, wavelet, x, levels, False)
            out["I_" + wp.case_key(1, i)] = lines(lib, wavelet, x, levels, True)
            cases.append({"dim": 1, "seed": seed, "wavelet": wavelet, "kind": kind, "n_lines": n_lines, "N": N, "levels": levels})
        for i, (seed, wavelet, kind, size_y, size_x, levels) in enumerate(wp.CASES_2D):
            x = wp.make_input(seed, kind, size_y, size_x, image=True)
            out["F_" + wp.case_key(2, i)] = image(lib, wavelet, x, levels, False)
            out["I_" + wp.case_key(2, i)] = image(lib, wavelet, x, levels, True)
            cases.append({"dim": 2, "seed": seed, "wavelet": wavelet, "kind": kind, "size_y": size_y, "size_x": size_x, "levels": levels})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(wp.GOLDEN, **out)
    with open(wp.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(wp.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_wp_golden.py",
                   "reference": "libdwt (src/libdwt.c line functions and one-level 2-D drivers per node; oracle/Makefile REF_CFLAGS)",
                   "files": {"wp.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", wp.GOLDEN, os.path.getsize(wp.GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
