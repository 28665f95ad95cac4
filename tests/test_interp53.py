"""CPU checks of the interpolating 5/3 wavelet: the numpy restatement of tests/interp53_model.py pinned bit for bit to
libdwt's own dwt_interp53_2f_s / _2i_s / _1f_s / _1i_s (oracle/_ref/libdwt_ref.so where it was built, the fixtures of
tests/golden/interp53.npz -- made from it by scripts/gen_interp53_golden.py -- everywhere), forward and inverse, 2-D
and 1-D, over the whole float range; the exported entries, their declarations and prototypes; the new wavelet id."""
import ctypes as C
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import interp53_model as M
from conftest import full_range_floats, same_floats

warnings.filterwarnings("ignore", category=RuntimeWarning)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interp53.npz")
ENTRIES = ["dwt_interp53_2f_s", "dwt_interp53_2i_s", "dwt_interp53_1f_s", "dwt_interp53_1i_s"]


def _golden():
    z = np.load(GOLDEN)
    two, one = [], []
    n = 0
    while "t%d_meta" % n in z:
        siy, six, j_max, d1, zp, j = (int(v) for v in z["t%d_meta" % n])
        two.append(dict(img=z["t%d_in" % n], fwd=z["t%d_fwd" % n], inv=z["t%d_inv" % n], size_i=None if siy < 0 else (siy, six),
                        j_max=j_max, d1=d1, zp=zp, j=j))
        n += 1
    n = 0
    while "o%d_meta" % n in z:
        si, j_max, zp, j = (int(v) for v in z["o%d_meta" % n])
        one.append(dict(x=z["o%d_in" % n], fwd=z["o%d_fwd" % n], inv=z["o%d_inv" % n], size_i=None if si < 0 else si,
                        j_max=j_max, zp=zp, j=j))
        n += 1
    return two, one


CASES_2D, CASES_1D = _golden()


def _ref():
    return M.RefInterp53() if os.path.exists(M.REF_SO) else None


REF = _ref()


def test_golden_covers_the_specified_cases():
    shapes = {c["img"].shape for c in CASES_2D}
    assert any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes)
    assert any(h % 2 and w % 2 for h, w in shapes) and any(h % 2 == 0 and w % 2 == 0 for h, w in shapes)
    assert any(c["size_i"] is not None for c in CASES_2D) and any(c["size_i"] is not None for c in CASES_1D)
    for key in ("d1", "zp"):
        assert {c[key] for c in CASES_2D} == {0, 1}
    assert {-1, 0, 40}.issubset({c["j_max"] for c in CASES_2D}) and {-1, 0, 40}.issubset({c["j_max"] for c in CASES_1D})
    assert any(not np.isfinite(c["img"]).all() for c in CASES_2D) and any(not np.isfinite(c["x"]).all() for c in CASES_1D)
    assert any(c["x"].shape[1] == 1 for c in CASES_1D)


@pytest.mark.parametrize("n", range(len(CASES_2D)))
def test_model_2d_matches_reference(n):
    c = CASES_2D[n]
    a = c["img"].copy()
    j = M.fwd2d(a, size_i=c["size_i"], j_max=c["j_max"], decompose_one=c["d1"], zero_padding=c["zp"])
    assert j == c["j"] and same_floats(a, c["fwd"])
    b = a.copy()
    M.inv2d(b, size_i=c["size_i"], j_max=j, decompose_one=c["d1"], zero_padding=c["zp"])
    assert same_floats(b, c["inv"])
    if REF is not None:
        r = c["img"].copy()
        assert REF.fwd2d(r, size_i=c["size_i"], j_max=c["j_max"], decompose_one=c["d1"], zero_padding=c["zp"]) == j
        assert same_floats(r, a)
        REF.inv2d(r, size_i=c["size_i"], j_max=j, decompose_one=c["d1"], zero_padding=c["zp"])
        assert same_floats(r, b)


@pytest.mark.parametrize("n", range(len(CASES_1D)))
def test_model_1d_matches_reference(n):
    c = CASES_1D[n]
    a = c["x"].copy()
    j = M.fwd1d(a, size_i=c["size_i"], j_max=c["j_max"], zero_padding=c["zp"])
    assert j == c["j"] and same_floats(a, c["fwd"])
    b = a.copy()
    M.inv1d(b, size_i=c["size_i"], j_max=j, zero_padding=c["zp"])
    assert same_floats(b, c["inv"])
    if REF is not None:
        r = c["x"].copy()
        assert REF.fwd1d(r, size_i=c["size_i"], j_max=c["j_max"], zero_padding=c["zp"]) == j
        assert same_floats(r, a)
        REF.inv1d(r, size_i=c["size_i"], j_max=j, zero_padding=c["zp"])
        assert same_floats(r, b)


def test_model_is_not_cdf53_with_a_zero_update():
    """c + 0 (l + r) is not c: an infinite neighbour makes it NaN and -0 becomes +0.  The even samples are only scaled."""
    t = M.fwd_lines(np.array([[1.0, np.inf, -0.0, 2.0]], np.float32))
    assert t[0, 0].view(np.uint32) == M.S1.view(np.uint32)
    assert t[0, 2] == 0 and np.signbit(t[0, 2])
    assert np.isinf(t[0, 1])


def test_model_round_trip_is_close():
    rng = np.random.default_rng(7)
    a = rng.random((33, 70), dtype=np.float32)
    b = a.copy()
    j = M.fwd2d(b)
    M.inv2d(b, j_max=j)
    assert np.allclose(a, b, atol=1e-5)
    x = rng.random((3, 129), dtype=np.float32)
    y = x.copy()
    j = M.fwd1d(y)
    M.inv1d(y, j_max=j)
    assert np.allclose(x, y, atol=1e-5)


def test_model_whole_float_range_runs():
    rng = np.random.default_rng(11)
    for klass in ("subnormal", "tiny", "huge", "mixed"):
        a = full_range_floats(rng, (20, 34), klass=klass, nonfinite=klass == "mixed")
        M.fwd2d(a.copy())
        M.fwd1d(a.copy())


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd

    return libdwt_amd


def test_library_exports_the_entries(dwt):
    for name in ENTRIES:
        assert hasattr(dwt.lib, name), name


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "libdwt.h")).read()
    for name in ENTRIES:
        assert name + "(" in text, name
    assert "DWT_HIP_INTERP53_S = 6" in open(os.path.join(ROOT, "include", "libdwt_hip.h")).read()


def test_header_declares_the_reference_types(tmp_path):
    """Each entry assigned to a pointer of the reference's type (src/libdwt.h:813, 1108, 1160, 1217): any difference in
    a parameter type is a compile error."""
    if not shutil.which("gcc"):
        pytest.skip("gcc is not installed")
    src = tmp_path / "types.c"
    src.write_text("""#include "libdwt.h"
typedef void (*fwd2_t)(void *, int, int, int, int, int, int, int *, int, int);
typedef void (*inv2_t)(void *, int, int, int, int, int, int, int, int, int);
typedef void (*fwd1_t)(void *, int, int, int, int *, int);
typedef void (*inv1_t)(void *, int, int, int, int, int);
fwd2_t f2 = dwt_interp53_2f_s;
inv2_t i2 = dwt_interp53_2i_s;
fwd1_t f1 = dwt_interp53_1f_s;
inv1_t i1 = dwt_interp53_1i_s;
""")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-o", str(tmp_path / "t.o"),
                        "-I", os.path.join(ROOT, "include")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_names(dwt):
    assert dwt.INTERP53_S == 6 and dwt.WAVELET_ID["interp53_s"] == 6
    assert dwt.FORWARD["interp53_s"] is dwt.dwt_interp53_2f_s and dwt.INVERSE["interp53_s"] is dwt.dwt_interp53_2i_s
    for name in ENTRIES:
        assert callable(getattr(dwt, name)), name


def test_entries_fail_loudly_without_gpu(dwt):
    if dwt.device_count() > 0:
        pytest.skip("a GPU is present")
    a = np.zeros((8, 8), np.float32)
    with pytest.raises(dwt.DwtError):
        dwt.dwt_interp53_2f_s(a, 32, 4, 8, 8, 8, 8)
    with pytest.raises(dwt.DwtError):
        dwt.transform1d_batch("interp53_s", 0, a, a, 32, 8, 8)
    assert not a.any()


def test_unknown_wavelets_are_rejected(dwt):
    a = np.zeros((8, 8), np.float32)
    j = C.c_int(-1)
    for w in (7, 10, -1):  # (8 and 9 are the int16 5/3 and the float 9/7 on binary16 storage)
        assert dwt.lib.dwt_hip_transform2d(w, 0, a.ctypes.data, a.ctypes.data, 32, 4, 8, 8, 8, 8, C.byref(j), 0, 0) != 0
        assert dwt.lib.dwt_hip_transform1d(w, 0, a.ctypes.data, a.ctypes.data, 4, 8, 8, C.byref(j), 0) != 0
    assert not a.any()
