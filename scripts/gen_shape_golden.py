#!/usr/bin/env python3
"""Writes tests/golden/shape.npz and tests/golden/shape_manifest.json: the results of the per-band coefficient operators,
the log / exp maps and the universal threshold for the cases of tests/shape_model.py.

The reference is loaded from oracle/_ref/libdwt_ref.so, where the build leaves it; no reference text or binary enters the
tree.  Before anything is written the generator ASSERTS, for every case:

1. the slot geometry of the model equals dwt_util_subband_s, address and sizes, for every slot;
2. SCALE and ZERO of the model equal dwt_util_scale_s and a memset of the band dwt_util_subband_s hands out, bit for bit;
3. the median behind the threshold equals dwt_util_abs_s + dwt_util_band_med_s on a copy of HH(1).

For COMPRESS, LOG and EXP the fixture holds the float64 model rounded once (what the GPU is held to within 1 ulp) AND the
host libm's powf / logf / expf values (what the reference's programs produce; the distance to them is measured).  The hdr
case holds the reference's own EAW 5/3 coefficients (alpha 0.8) of the log luminance.

    python scripts/gen_shape_golden.py
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eaw_model  # noqa: E402
import shape_model as sm  # noqa: E402

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdwt_ref.so")
F32 = np.float32
BAND_OF_SLOT = (1, 2, 3)  # enum dwt_subbands: DWT_LL 0, DWT_HL 1, DWT_LH 2, DWT_HH 3


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def bind(lib):
    I, P, F = C.c_int, C.c_void_p, C.c_float
    lib.dwt_util_subband_s.argtypes = [P, I, I, I, I, I, I, I, I, C.POINTER(P), C.POINTER(I), C.POINTER(I)]
    lib.dwt_util_subband_s.restype = None
    lib.dwt_util_scale_s.argtypes = [P, I, I, I, I, F]
    lib.dwt_util_abs_s.argtypes = [P, I, I, I, I]
    lib.dwt_util_abs_s.restype = None
    lib.dwt_util_band_med_s.argtypes = [P, I, I, I, I]
    lib.dwt_util_band_med_s.restype = F


def ref_band(lib, img, sox, soy, six, siy, j, band):
    """(byte offset, size_x, size_y) of a band as the reference hands it out"""
    q, w, h = C.c_void_p(), C.c_int(), C.c_int()
    lib.dwt_util_subband_s(img.ctypes.data, img.strides[0], 4, sox, soy, six, siy, j, band, C.byref(q), C.byref(w), C.byref(h))
    return q.value - img.ctypes.data, w.value, h.value


def check_case(lib, name, out):
    sox, soy, six, siy, j_max, kind = sm.CASES[name]
    x, J, ops, params = sm.case_arrays(name)
    tag = "case %s" % name
    geo = sm.slots(sox, soy, six, siy, J)
    # 1. geometry
    for k, (x0, y0, w, h) in enumerate(geo):
        j, band = (k // 3 + 1, BAND_OF_SLOT[k % 3]) if k < 3 * J else (J, 0)
        off, rw, rh = ref_band(lib, x, sox, soy, six, siy, j, band)
        assert (rw, rh) == (w, h) and (off == y0 * x.strides[0] + 4 * x0 or not (w and h)), "geometry: model != reference, %s slot %d" % (tag, k)
    # 2. SCALE and ZERO through the reference, slot by slot
    for op in (sm.SCALE, sm.ZERO):
        for k, (x0, y0, w, h) in enumerate(geo):
            if not (w and h):
                continue
            one = np.zeros(len(geo), np.int32)
            one[k] = op
            want = x.copy()
            j, band = (k // 3 + 1, BAND_OF_SLOT[k % 3]) if k < 3 * J else (J, 0)
            off, rw, rh = ref_band(lib, want, sox, soy, six, siy, j, band)
            if op == sm.SCALE:
                lib.dwt_util_scale_s(want.ctypes.data + off, rw, rh, want.strides[0], 4, sm.PARAM[sm.SCALE])
            else:
                for y in range(rh):
                    C.memset(want.ctypes.data + off + y * want.strides[0], 0, 4 * rw)
            got = sm.apply_table(x, sox, soy, six, siy, J, one, np.full(len(geo), sm.PARAM[op], F32))
            assert np.array_equal(bits(got), bits(want)), "%s: model != reference, %s slot %d" % (sm.OP_NAMES[op], tag, k)
    # the case's own table: float64 model, and libm where COMPRESS is part of it
    out[name + ".geometry"] = np.array(geo, np.int32)
    out[name + ".ops"], out[name + ".params"] = ops, params
    out[name + ".out"] = sm.apply_table(x, sox, soy, six, siy, J, ops, params)
    if sm.COMPRESS in ops:
        out[name + ".libm"] = sm.apply_table(x, sox, soy, six, siy, J, ops, params, how="libm")
    # 3. the threshold's median
    if sox // 2 and soy // 2:
        xin = sm.threshold_input(x, sox, soy)  # (no NaN in HH(1): the reference's comparator is no order there)
        mag = np.ascontiguousarray(sm.hh1(xin, sox, soy)).copy()
        lib.dwt_util_abs_s(mag.ctypes.data, mag.strides[0], 4, mag.shape[1], mag.shape[0])
        med = F32(lib.dwt_util_band_med_s(mag.ctypes.data, mag.strides[0], 4, mag.shape[1], mag.shape[0]))
        assert bits(med) == bits(sm.abs_median(sm.hh1(xin, sox, soy))), "median magnitude: model != reference, " + tag
        out[name + ".lambda"] = sm.threshold(xin, sox, soy)
    return {"name": name, "size_o": [sox, soy], "size_i": [six, siy], "j_max": j_max, "levels": J, "table": kind, "seed": sm.case_seed(name)}


def main():
    assert os.path.exists(REF_SO), "build the reference first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = C.CDLL(REF_SO)
    bind(lib)
    out, cases = {}, []
    for name in sm.CASES:
        cases.append(check_case(lib, name, out))
    # the maps over one input with every special value
    m = sm.make_input(99, 13, 21)
    for op, a in ((sm.LOG, 1e-5), (sm.EXP, 1e-5)):
        out["map.%s" % op] = sm.apply_op(m, op, a)
        out["map.%s.libm" % op] = sm.apply_op(m, op, a, how="libm")
    # the hdr flow: the reference's EAW 5/3 coefficients (alpha 0.8) of the log luminance
    sox, soy = sm.CASES["hdr"][:2]
    loglum = sm.apply_op(sm.hdr_input(soy, sox), sm.LOG, 1e-5)
    coef = loglum.copy()
    j, _, _ = eaw_model.RefEaw().fwd(coef, alpha=0.8)
    assert j == sm.levels(sox, soy, -1), "the EAW forward and the band entries must agree on the default level count"
    ops, params = sm.make_table("compress", 3 * j + 1)
    out["hdr.log"], out["hdr.eaw"] = loglum, coef
    out["hdr.compressed"] = sm.apply_table(coef, sox, soy, sox, soy, j, ops, params)
    out["hdr.compressed.libm"] = sm.apply_table(coef, sox, soy, sox, soy, j, ops, params, how="libm")
    np.savez_compressed(sm.GOLDEN, **out)
    with open(sm.GOLDEN, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(sm.MANIFEST, "w") as f:
        json.dump({"generator": "scripts/gen_shape_golden.py", "reference": "oracle/_ref/libdwt_ref.so (oracle/Makefile REF_CFLAGS)",
                   "asserted": "slot geometry == dwt_util_subband_s; SCALE == dwt_util_scale_s and ZERO == memset of every band, bit for bit; "
                               "median magnitude of HH(1) == dwt_util_abs_s + dwt_util_band_med_s",
                   "files": {"shape.npz": {"sha256": sha, "cases": cases}}}, f, indent=1)
        f.write("\n")
    print("wrote", sm.GOLDEN, os.path.getsize(sm.GOLDEN), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
