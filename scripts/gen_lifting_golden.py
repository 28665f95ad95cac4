#!/usr/bin/env python3
"""Writes tests/golden/lifting.npz and tests/golden/lifting_manifest.json: the reference's Daubechies D4 and Haar cores on
random float images, one level, subbands interleaved in place (examples/cores/cores-d4.c: fdwt2_d4_sep_horiz /
idwt2_d4_sep_horiz; examples/cores/cores-haar.c: cores2f_haar_v2x2_f32 / cores2i_haar_v2x2_f32).

Per case the file holds the input, the forward core's output and the inverse core's output OF that output.  The generator
ASSERTS that the reference equals tests/lifting_model.py (builtin "D4" / "HAAR", one level in sample order) bit for bit and
fails otherwise.  What is compared follows from the cores' text, not from trial:
  * D4: only SQUARE images (the reference's column loop runs to size_y), and only the samples at least MARGIN = 4 away from
    every border -- the reference truncates its steps at the borders (its loops skip the targets whose tap lies outside)
    where the model reflects, and a truncated target reaches 3 samples into a line through the steps behind it.
  * Haar: even sizes, the whole frame -- a 2 x 2 block needs no border.  The core is the 2 x 1 element step applied along
    x, then along y (and undone in the same order), which is what the model's level does.

The reference's sources are compiled from where they lie with the reference's own release flags into a temporary
directory outside the repository, loaded from there, and the directory is deleted: no reference text or binary enters
the tree.

    python scripts/gen_lifting_golden.py [--ref /path/to/libdwt]
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
import lifting_model as M  # noqa: E402
from gen_swt_golden import ref_cflags  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "lifting.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "lifting_manifest.json")
MARGIN = 4
D4_SIZES = [32, 64]
HAAR_SHAPES = [(2, 2), (6, 10), (32, 32), (48, 64)]  # (rows, columns), even


class image_t(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("size_x", C.c_int), ("size_y", C.c_int), ("stride_x", C.c_int), ("stride_y", C.c_int),
                ("size", C.c_int)]


def run_core(fn, img):
    src = np.ascontiguousarray(img, np.float32)
    dst = np.zeros_like(src)
    h, w = src.shape
    s = image_t(src.ctypes.data, w, h, 4, src.strides[0], 0)
    d = image_t(dst.ctypes.data, w, h, 4, dst.strides[0], 0)
    fn(C.byref(s), C.byref(d))
    return dst


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def model_level(scheme, x, inverse):
    r = np.array(x, np.float32, ndmin=3, copy=True)
    M.level2d(scheme, r, inverse)
    return r[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src, cores = os.path.join(args.ref, "src"), os.path.join(args.ref, "examples", "cores")
    tmp = tempfile.mkdtemp(prefix="lifting_golden_")
    try:
        so = os.path.join(tmp, "libcores_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-I" + cores, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(cores, f) for f in ("cores-d4.c", "cores-haar.c", "coords.c")] +
                              [os.path.join(src, f) for f in ("libdwt.c", "system.c", "image.c")] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        fns = {n: getattr(lib, n) for n in ("fdwt2_d4_sep_horiz", "idwt2_d4_sep_horiz", "cores2f_haar_v2x2_f32", "cores2i_haar_v2x2_f32")}
        for fn in fns.values():
            fn.argtypes = [C.POINTER(image_t), C.POINTER(image_t)]
            fn.restype = None
        rng = np.random.default_rng(3307)
        out, cases = {}, []
        d4, haar = M.builtin("D4"), M.builtin("HAAR")
        m = MARGIN
        for n in D4_SIZES:
            key = "d4_%d" % n
            x = rng.uniform(-1, 1, (n, n)).astype(np.float32)
            fwd = run_core(fns["fdwt2_d4_sep_horiz"], x)
            inv = run_core(fns["idwt2_d4_sep_horiz"], fwd)
            assert same(model_level(d4, x, False)[m:-m, m:-m], fwd[m:-m, m:-m]), ("reference != model", key, "forward")
            assert same(model_level(d4, fwd, True)[m:-m, m:-m], inv[m:-m, m:-m]), ("reference != model", key, "inverse")
            assert not same(model_level(d4, x, False), fwd), "the borders were expected to differ (truncated against reflected steps)"
            out[key + "_in"], out[key + "_fwd"], out[key + "_inv"] = x, fwd, inv
            cases.append({"core": "d4", "key": key, "size": n, "rows": n, "columns": n})
        for h, w in HAAR_SHAPES:
            key = "haar_%dx%d" % (h, w)
            x = rng.uniform(-1, 1, (h, w)).astype(np.float32)
            fwd = run_core(fns["cores2f_haar_v2x2_f32"], x)
            inv = run_core(fns["cores2i_haar_v2x2_f32"], fwd)
            assert same(model_level(haar, x, False), fwd), ("reference != model", key, "forward")
            assert same(model_level(haar, fwd, True), inv), ("reference != model", key, "inverse")
            out[key + "_in"], out[key + "_fwd"], out[key + "_inv"] = x, fwd, inv
            cases.append({"core": "haar", "key": key, "size": None, "rows": h, "columns": w})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(GOLDEN, **out)
    with open(GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_lifting_golden.py",
                   "reference": "libdwt (examples/cores/cores-d4.c: fdwt2_d4_sep_horiz, idwt2_d4_sep_horiz; examples/cores/cores-haar.c: "
                                "cores2f_haar_v2x2_f32, cores2i_haar_v2x2_f32; oracle/Makefile REF_CFLAGS)",
                   "asserted": "reference == tests/lifting_model.py on every case: D4 at least `margin` samples away from every border, Haar everywhere",
                   "margin": MARGIN,
                   "haar_left_out": None,
                   "left_out_by_rule": {"d4_borders": "the reference truncates the steps at the borders, the library reflects every tap",
                                        "d4_not_square": "the reference's column loop runs to size_y",
                                        "haar_odd": "odd sizes: a 2 x 2 block would need a border rule"},
                   "sha256": sha, "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
