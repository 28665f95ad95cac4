#!/usr/bin/env python3
"""Writes tests/golden/condition.npz and tests/golden/condition_manifest.json: what the reference's conditioning
functions (dwt_util_get_center1_s, _shift21_med_s, _center21_s, _scale21_s, _find_min_max_s, _displace1_s,
_displace1_zero_s; src/libdwt.c:25426-26055) give for the cases of tests/condition_model.py.

The reference is loaded from oracle/_ref/libdwt_ref.so where the build left it; otherwise its libdwt.c is compiled from
where it lies with the reference's own release flags into a temporary directory outside the repository, loaded from
there, and the directory is deleted: no reference text or binary enters the tree.

The generator ASSERTS that the numpy model equals the reference on every row of every case -- centres, rows after each
operation, extrema, displacements -- and writes nothing otherwise (contract part 3).  A seed whose data
holds a near-tie row (a 1-ulp powf difference flips a comparison) is to be changed in condition_model.py and recorded
under "moved_seeds" below; no row may be left out.

    python scripts/gen_condition_golden.py [--ref /path/to/libdwt]
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
import condition_model as cm  # noqa: E402

REF_SRCS = ["libdwt.c", "system.c"]
MOVED_SEEDS = []  # [{"case": ..., "from": seed, "to": seed, "why": ...}]


def ref_cflags(ref):
    version = open(os.path.join(ref, "VERSION")).read().strip() if os.path.exists(os.path.join(ref, "VERSION")) else ""
    return ["-std=c99", "-O3", "-ftree-vectorize", "-fopenmp", "-fPIC", "-finline-functions", "-DNDEBUG",
            "-D_POSIX_C_SOURCE=199309L", "-D_GNU_SOURCE", '-DPACKAGE_VERSION="%s"' % version, '-DPACKAGE_NAME="libdwt"',
            '-DPACKAGE_STRING="libdwt %s"' % version, '-DARCH="x86_64"', "-w"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, but zeros by value: which of +0 / -0 a median stands for is unspecified"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | ((a == 0) & (b == 0))))


def run(lib):
    _I, _P, _F = C.c_int, C.c_void_p, C.c_float
    lib.dwt_util_get_center1_s.argtypes = [_P, _I, _I]
    lib.dwt_util_get_center1_s.restype = _I
    lib.dwt_util_shift21_med_s.argtypes = [_P, _I, _I, _I, _I]
    lib.dwt_util_shift21_med_s.restype = None
    lib.dwt_util_center21_s.argtypes = [_P, _I, _I, _I, _I, _I]
    lib.dwt_util_scale21_s.argtypes = [_P, _I, _I, _I, _I, _F, _F]
    lib.dwt_util_find_min_max_s.argtypes = [_P, _I, _I, _I, _I, _P, _P]
    for name in ("dwt_util_displace1_s", "dwt_util_displace1_zero_s"):
        getattr(lib, name).argtypes = [_P, _I, _I, _I]
    out, cases = {}, []
    for i, (seed, kind, n_lines, n) in enumerate(cm.CASES):
        x = cm.make_input(seed, kind, n_lines, n)
        tag = "%s n=%d seed=%d" % (kind, n, seed)
        centre = np.array([lib.dwt_util_get_center1_s(x[y].ctypes.data, n, 4) for y in range(n_lines)], np.int32)
        assert np.array_equal(centre, [cm.get_center1(r) for r in x]), "centre: model != reference, " + tag
        shifted = x.copy()
        lib.dwt_util_shift21_med_s(shifted.ctypes.data, n, n_lines, 4 * n, 4)
        m, _ = cm.condition(x, cm.MED_SHIFT)
        assert same(m, shifted), "median shift: model != reference, " + tag
        centred = shifted.copy()
        lib.dwt_util_center21_s(centred.ctypes.data, n, n_lines, 4 * n, 4, 20)
        m, info = cm.condition(x, cm.MED_SHIFT | cm.CENTER, 20)
        assert same(m, centred), "centring: model != reference, " + tag
        scaled = centred.copy()
        lib.dwt_util_scale21_s(scaled.ctypes.data, n, n_lines, 4 * n, 4, 0.0, 1.0)
        m, _ = cm.condition(x, cm.MED_SHIFT | cm.CENTER | cm.SCALE, 20, 0.0, 1.0)
        assert same(m, scaled), "scaling: model != reference, " + tag
        mn, mx = np.zeros(n_lines, np.float32), np.zeros(n_lines, np.float32)
        for y in range(n_lines):
            lib.dwt_util_find_min_max_s(x[y].ctypes.data, n, 1, 4 * n, 4, mn[y:].ctypes.data, mx[y:].ctypes.data)
            assert (mn[y], mx[y]) == cm.min_max(x[y]), "min / max: model != reference, " + tag
        out["center_%d" % i], out["shift_%d" % i], out["centered_%d" % i], out["scaled_%d" % i] = centre, shifted, centred, scaled
        out["min_%d" % i], out["max_%d" % i], out["info_%d" % i] = mn, mx, info
        displaced = n <= 65 and kind == "spectrum"
        if displaced:
            for zero, name in ((0, "dwt_util_displace1_s"), (1, "dwt_util_displace1_zero_s")):
                rows = np.zeros((len(cm.DISPLACEMENTS), n_lines, n), np.float32)
                for k, dn in enumerate(cm.DISPLACEMENTS):
                    d = cm.displacement(dn, n)
                    rows[k] = x
                    for y in range(n_lines):
                        getattr(lib, name)(rows[k, y].ctypes.data, n, 4, d)
                        assert np.array_equal(bits(rows[k, y]), bits(cm.displace1(x[y], d, zero))), "displace: model != reference, " + tag
                out["displace%d_%d" % (zero, i)] = rows
        cases.append({"seed": seed, "kind": kind, "n_lines": n_lines, "n": n, "displaced": displaced})
    return out, cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    built = os.path.join(ROOT, "oracle", "_ref", "libdwt_ref.so")
    tmp = None
    try:
        if os.path.exists(built):
            lib = C.CDLL(built)
            how = "oracle/_ref/libdwt_ref.so (oracle/Makefile REF_CFLAGS)"
        else:
            src = os.path.join(args.ref, "src")
            tmp = tempfile.mkdtemp(prefix="condition_golden_")
            so = os.path.join(tmp, "libcond_ref.so")
            subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                                  [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
            lib = C.CDLL(so)
            how = "libdwt (src/libdwt.c, src/system.c; oracle/Makefile REF_CFLAGS)"
        out, cases = run(lib)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(cm.GOLDEN, **out)
    with open(cm.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(cm.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_condition_golden.py", "reference": how,
                   "asserted": "model == reference on every row of every case: centres, rows after shift21_med, center21(20), scale21(0, 1), min / max, displacements",
                   "moved_seeds": MOVED_SEEDS, "files": {"condition.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", cm.GOLDEN, os.path.getsize(cm.GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
