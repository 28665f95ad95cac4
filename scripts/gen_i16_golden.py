#!/usr/bin/env python3
"""Writes tests/golden/cdf53_i16.npz and tests/golden/cdf53_i16_manifest.json: the reference's int16 5/3 cores
cores2f_cdf53_v2x2_i16 / cores2i_cdf53_v2x2_i16 (examples/cores/cores.c: "JPEG 2000 compatible, F.3.8.1 Reversible 1D
filtering, F.3.2 2D_SD") on random int16 images.

A core does ONE level and leaves it interleaved in place.  Per case the file holds the input and the core's output; the
multi-level cases re-apply the core to the de-interleaved LL band and hold every level's output.  The generator ASSERTS
that the reference equals tests/i16_model.py on every case and fails otherwise: the cases stay inside the domain where
the reference evaluates the exact arithmetic (|x| <= 4096 for one level, <= 1024 for several -- its compiled forward
variant leaves the arithmetic from about +-8191 on), and the shapes the reference gets wrong are left out BY RULE, not
by trial: inverses of an odd size or with a side below 4, and every shape with a one-line direction.

The reference's examples/cores/{cores.c,coords.c,fix.c} and src/{libdwt.c,system.c,image.c} are compiled from where they
lie with the reference's own release flags into a temporary directory outside the repository, loaded from there, and
the directory is deleted: no reference text or binary enters the tree.

    python scripts/gen_i16_golden.py [--ref /path/to/libdwt]
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
import i16_model as M  # noqa: E402
from gen_swt_golden import ref_cflags  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "cdf53_i16.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "cdf53_i16_manifest.json")

FWD_SHAPES = [(2, 2), (3, 3), (2, 5), (9, 14), (13, 7), (16, 12), (32, 32), (67, 130)]  # (rows, columns)
MULTI = [((32, 32), 2), ((32, 32), 3), ((67, 130), 2), ((67, 130), 3), ((16, 12), 2)]
INV_SHAPES = [(4, 4), (6, 10), (8, 8), (16, 12), (32, 32), (66, 130)]
LEFT_OUT = {
    "inverse": "odd sizes and sizes with a side below 4: the reference's inverse core is wrong there (2x2, 2x8, every odd size)",
    "one_line": "1 x N and N x 1 images: the reference's cores do not follow the plain rule on a one-line direction",
    "range": "|x| > 4096 (one level) / > 1024 (several): the compiled forward variant leaves the exact arithmetic near +-8191",
}


class image_t(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("size_x", C.c_int), ("size_y", C.c_int), ("stride_x", C.c_int), ("stride_y", C.c_int),
                ("size", C.c_int)]


def run_core(fn, img):
    src = np.ascontiguousarray(img, np.int16)
    dst = np.zeros_like(src)
    h, w = src.shape
    s = image_t(src.ctypes.data, w, h, 2, src.strides[0], 0)
    d = image_t(dst.ctypes.data, w, h, 2, dst.strides[0], 0)
    fn(C.byref(s), C.byref(d))
    return dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src, cores = os.path.join(args.ref, "src"), os.path.join(args.ref, "examples", "cores")
    tmp = tempfile.mkdtemp(prefix="i16_golden_")
    try:
        so = os.path.join(tmp, "libcores_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-I" + cores, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(cores, f) for f in ("cores.c", "coords.c", "fix.c")] +
                              [os.path.join(src, f) for f in ("libdwt.c", "system.c", "image.c")] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        fwd, inv = lib.cores2f_cdf53_v2x2_i16, lib.cores2i_cdf53_v2x2_i16
        for fn in (fwd, inv):
            fn.argtypes = [C.POINTER(image_t), C.POINTER(image_t)]
            fn.restype = None
        rng = np.random.default_rng(1653)
        out, cases = {}, []

        def add(kind, shape, levels, amp):
            i = len(cases)
            x = rng.integers(-amp, amp + 1, size=shape).astype(np.int16)
            out["in_%d" % i] = x
            cur = x
            for l in range(levels):
                if kind == "inverse":
                    coef = M.core_fwd(cur)
                    got = run_core(inv, coef)
                    assert np.array_equal(got, M.core_inv(coef)) and np.array_equal(got, cur), ("reference != model", kind, shape, l)
                    out["in_%d" % i] = coef
                else:
                    got = run_core(fwd, cur)
                    assert np.array_equal(got, M.core_fwd(cur)), ("reference != model", kind, shape, l)
                out["out_%d_%d" % (i, l)] = got
                cur = np.ascontiguousarray(got[0::2, 0::2])
            cases.append({"kind": kind, "rows": shape[0], "columns": shape[1], "levels": levels, "amplitude": amp})

        for shape in FWD_SHAPES:
            add("forward", shape, 1, 4096)
            add("forward", shape, 1, 256)
        for shape, levels in MULTI:
            add("forward", shape, levels, 1024)
        for shape in INV_SHAPES:
            add("inverse", shape, 1, 4096)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(GOLDEN, **out)
    with open(GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_i16_golden.py",
                   "reference": "libdwt (examples/cores/cores.c: cores2f_cdf53_v2x2_i16, cores2i_cdf53_v2x2_i16; oracle/Makefile REF_CFLAGS)",
                   "asserted": "reference == tests/i16_model.py on every case",
                   "left_out_by_rule": LEFT_OUT,
                   "files": {"cdf53_i16.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
