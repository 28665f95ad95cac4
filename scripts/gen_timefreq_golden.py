#!/usr/bin/env python3
"""Writes tests/golden/timefreq.npz and tests/golden/timefreq_manifest.json: for the cases of tests/timefreq_model.py the
input, the reference's kernels (gabor_gen_kernel / s_gen_kernel), the complex sums of dwt_util_cdot1_s, the planes of
gabor_{ft,wt,st}_s and their _arg_ twins, and phase_derivative_s / detect_ridges{1,2,3}_s over the reference's own planes.

The reference's gabor.c, libdwt.c and system.c are compiled from where they lie with the reference's own release flags
(oracle/Makefile: REF_CFLAGS) into a temporary directory outside the repository, loaded from there, and the directory is
deleted: no reference text or binary enters the tree.

The manifest also records what the tests take their allowances from: the largest error of the reference's cargf against
float64 atan2 of the same (re, im), the largest difference between the reference's taps and the built library's
generators on this host (in float32 ulps), and the smallest distance of a detect_ridges3_s direction from its +-1/2
thresholds, which must stay above 2^-20 (the script fails otherwise: choose another seed).

    python scripts/gen_timefreq_golden.py [--ref /path/to/libdwt]
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
sys.path.insert(0, ROOT)
import timefreq_model as tm  # noqa: E402
from gen_swt_golden import ref_cflags  # noqa: E402

REF_SRCS = ["gabor.c", "libdwt.c", "system.c"]
F32 = np.float32
_F, _I, _P = C.c_float, C.c_int, C.c_void_p


def bin_params(kind, y, bins, sigma, freq, lib):
    """(sigma, frequency, scale) of bin y, float32 operation by operation as gabor_{ft,wt,st}_s derive them"""
    norm1 = F32(F32(y + 1) / F32(bins))
    if kind == "ft":
        return F32(sigma), F32(F32(F32(y) / F32(bins)) * F32(1) * tm.PI), F32(1)
    if kind == "wt":
        f = F32(F32(F32(norm1 * F32(0.5)) * F32(2)) * tm.PI)
        return F32(sigma), F32(freq), F32(F32(freq) / f)
    f = F32(norm1 * F32(0.5))
    return F32(lib.s_sigma(f)), f, F32(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    args = ap.parse_args()
    src = os.path.join(args.ref, "src")
    tmp = tempfile.mkdtemp(prefix="timefreq_golden_")
    try:
        so = os.path.join(tmp, "libgabor_ref.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + ref_cflags(args.ref) + ["-I" + src, "-shared", "-Wl,-Bsymbolic", "-o", so] +
                              [os.path.join(src, f) for f in REF_SRCS] + ["-lm", "-lrt"])
        lib = C.CDLL(so)
        libc = C.CDLL(None)
        libc.free.argtypes = [_P]
        lib.s_sigma.argtypes, lib.s_sigma.restype = [_F], _F
        lib.gaussian_size.argtypes, lib.gaussian_size.restype = [_F, _F], _I
        lib.gabor_gen_kernel.argtypes, lib.gabor_gen_kernel.restype = [C.POINTER(_P), _I, _F, _F, _F], None
        lib.s_gen_kernel.argtypes, lib.s_gen_kernel.restype = [C.POINTER(_P), _I, _F], None
        # a float complex comes back in xmm0 as two packed floats: read it as the eight bytes of a double
        lib.dwt_util_cdot1_s.argtypes, lib.dwt_util_cdot1_s.restype = [_P, _I, _I, _I, _P, _I, _I, _I], C.c_double
        for name in ("gabor_ft_s", "gabor_ft_arg_s"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [_P, _I, _I, _P, _I, _I, _I, _F], None
        for name in ("gabor_wt_s", "gabor_wt_arg_s"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [_P, _I, _I, _P, _I, _I, _I, _F, _F], None
        for name in ("gabor_st_s", "gabor_st_arg_s"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [_P, _I, _I, _P, _I, _I, _I], None
        for name in ("phase_derivative_s", "detect_ridges1_s", "detect_ridges2_s", "detect_ridges3_s"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [_P, _P, _I, _I, _I, _I, _F], None
        import libdwt_amd as dwt

        out, cases = {}, []
        arg_ulp, tap_ulp, margin = 0.0, 0.0, np.inf
        for i, (seed, kind, inp, n, bins, sigma, freq) in enumerate(tm.CASES):
            x = np.ascontiguousarray(tm.make_input(seed, inp, 1, n)[0])
            sizes, centers, taps = np.zeros(bins, np.int32), np.zeros(bins, np.int32), []
            dots = np.zeros((bins, n, 2), F32)
            for y in range(bins):
                sg, f, a = bin_params(kind, y, bins, sigma, freq, lib)
                k = _P(None)
                if kind == "st":
                    lib.s_gen_kernel(C.byref(k), 8, f)
                else:
                    lib.gabor_gen_kernel(C.byref(k), 8, sg, f, a)
                sizes[y] = lib.gaussian_size(sg, a)
                centers[y] = sizes[y] // 2
                taps.append(np.ctypeslib.as_array(C.cast(k, C.POINTER(_F)), (2 * int(sizes[y]),)).copy().view(np.complex64))
                for t in range(n):
                    v = lib.dwt_util_cdot1_s(x.ctypes.data, n, 4, t, k, int(sizes[y]), 8, int(centers[y]))
                    dots[bins - 1 - y, t] = np.array([v], np.float64).view(F32)
                libc.free(k)
            mag, arg = np.zeros((bins, n), F32), np.zeros((bins, n), F32)
            extra = {"ft": (F32(sigma),), "wt": (F32(sigma), F32(freq)), "st": ()}[kind]
            getattr(lib, "gabor_%s_s" % kind)(x.ctypes.data, 4, n, mag.ctypes.data, n * 4, 4, bins, *extra)
            getattr(lib, "gabor_%s_arg_s" % kind)(x.ctypes.data, 4, n, arg.ctypes.data, n * 4, 4, bins, *extra)
            # the kernels above are the ones the transforms generate for themselves, and the model restates both
            assert tm.same(tm.magnitude(dots[..., 0], dots[..., 1]), mag), ("magnitude", i)
            re, im, mmag = tm.planes(x, sizes, centers, taps)
            assert tm.same(re, dots[..., 0]) and tm.same(im, dots[..., 1]) and tm.same(mmag, mag), ("model", i)
            ops = {}
            for name, fn, source, param in (("pd", "phase_derivative_s", arg, tm.LIMIT), ("r1", "detect_ridges1_s", mag, 0.0)):
                ops[name] = np.zeros((bins, n), F32)
                getattr(lib, fn)(source.ctypes.data, ops[name].ctypes.data, n * 4, 4, n, bins, param)
            for name, fn, source in (("r2", "detect_ridges2_s", ops["pd"]), ("r3", "detect_ridges3_s", mag)):
                ops[name] = np.zeros((bins, n), F32)
                getattr(lib, fn)(source.ctypes.data, ops[name].ctypes.data, n * 4, 4, n, bins, 0.0)
            margin = min(margin, tm.ridges3_margin(mag))
            with np.errstate(all="ignore"):
                e = tm.ulps(arg, np.arctan2(dots[..., 1].astype(np.float64), dots[..., 0].astype(np.float64)))
            if np.isfinite(e).any():
                arg_ulp = max(arg_ulp, float(np.nanmax(e[np.isfinite(e)])))
            # the built library's generators on this host against the reference's taps
            bank = dwt.timefreq_bank(kind, bins, sigma, freq)
            s2, c2, t2 = bank.query()
            bank.free()
            assert np.array_equal(s2, sizes) and np.array_equal(c2, centers), ("sizes", i)
            for y in range(bins):
                for part in (np.real, np.imag):
                    d = tm.ulps(part(t2[y]), part(taps[y]).astype(np.float64))
                    tap_ulp = max(tap_ulp, float(d.max()))
            out.update({"x_%d" % i: x, "sizes_%d" % i: sizes, "centers_%d" % i: centers, "taps_%d" % i: np.concatenate(taps),
                        "dots_%d" % i: dots, "mag_%d" % i: mag, "arg_%d" % i: arg})
            out.update({"%s_%d" % (k, i): v for k, v in ops.items()})
            cases.append({"seed": seed, "kind": kind, "input": inp, "n": n, "bins": bins, "sigma": sigma, "freq": freq})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert margin > 2.0 ** -20, ("a detect_ridges3_s direction within 2^-20 of its threshold: choose other seeds", margin)
    np.savez_compressed(tm.GOLDEN, **out)
    with open(tm.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(tm.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_timefreq_golden.py", "reference": "libdwt (src/gabor.c, src/libdwt.c, src/system.c; oracle/Makefile REF_CFLAGS)",
                   "arg_ref_max_ulp": arg_ulp, "tap_max_ulp": tap_ulp, "ridges3_min_margin": margin, "ridges3_excluded_points": 0,
                   "phase_limit": tm.LIMIT, "files": {"timefreq.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", tm.GOLDEN, os.path.getsize(tm.GOLDEN), "bytes,", len(cases), "cases; arg", arg_ulp, "ulp, taps", tap_ulp, "ulp, margin", margin)


if __name__ == "__main__":
    main()
