"""CPU checks of the stationary wavelet transform: the numpy float32 restatement (tests/swt_model.py) against the outputs of
the reference's two functions (tests/golden/swt.npz, written by scripts/gen_swt_golden.py), the ABI of the built library,
the argument checks, and a call without a device."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import swt_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(sm.GOLDEN)
F32 = np.float32


def test_manifest():
    with open(sm.MANIFEST) as f:
        info = json.load(f)["files"]["swt.npz"]
    with open(sm.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == info["sha256"]
    assert [(c["seed"], c["wavelet"], c["kind"], c["n"], c["levels"]) for c in info["cases"]] == sm.CASES
    assert os.path.getsize(sm.GOLDEN) < 1 << 20


@pytest.mark.parametrize("i", range(len(sm.CASES)))
def test_restatement_equals_golden(i):
    seed, wavelet, kind, n, levels = sm.CASES[i]
    L, H = sm.swt_levels(sm.make_input(seed, kind, 1, n)[0], wavelet, levels)
    assert GOLD["L_%d" % i].shape == (levels, n)
    assert sm.same(L, GOLD["L_%d" % i]) and sm.same(H, GOLD["H_%d" % i])


def test_restatement_properties():
    """what the definition implies, checked on the restatement itself: a constant row passes the low-pass filter scaled by
    the sum of its taps and gives (nearly) zero detail; a dilation beyond the row leaves only the ends and the centre."""
    for w in sm.WAVELETS:
        gl, gh = sm.FILTERS[w]
        assert len(gl) == len(gh) + 2 and np.array_equal(gl, gl[::-1]) and np.array_equal(gh, gh[::-1])
        x = np.arange(5, dtype=F32)
        L, H = sm.swt_level(x, w, 10)  # every tap but the centre one clamps to an end
        c = len(gl) // 2
        want = F32(0)
        for k in range(-c, c + 1):
            want = F32(want + F32((x[-1] if k < 0 else x[0] if k > 0 else x[2]) * gl[k + c]))
        assert L[2] == want
    batch = sm.make_input(1, "normal", 3, 50)
    L, H = sm.swt_levels(batch, "cdf97_s", 4)
    for y in range(3):
        Ly, Hy = sm.swt_levels(batch[y], "cdf97_s", 4)
        assert sm.same(L[:, y], Ly) and sm.same(H[:, y], Hy)


NEW_SYMBOLS = ["dwt_hip_swt1d_batch", "dwt_hip_swt1d_level", "dwt_hip_swt_features1d_batch"]


def test_abi_exports():
    lib = C.CDLL(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so"))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    import libdwt_amd as dwt

    for s in ["swt1d_batch", "swt_features1d_batch", "swt_cdf97_f_ex_stride_s", "swt_cdf53_f_ex_stride_s"]:
        assert callable(getattr(dwt, s)), s
    assert dwt.SWT_MAX_LEVELS == sm.MAX_LEVELS == 24


def test_swt_header_compiles_and_links(tmp_path):
    """include/swt.h gives the reference's two prototypes as inline wrappers: a caller written against src/swt.h compiles
    (C99 and C++) and links against the library with nothing but the header"""
    import subprocess

    src = tmp_path / "t.c"
    src.write_text('#include "swt.h"\nint main(int argc, char **argv){float x[8]={0},l[8],h[8];(void)argv;if(argc>99){'
                   'swt_cdf97_f_ex_stride_s(x,l,h,8,sizeof(float),0);swt_cdf53_f_ex_stride_s(x,l,h,8,sizeof(float),1);}return 0;}\n')
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-l:libdwt_hip.so", "-Wl,-rpath," + libdir])
    subprocess.check_call(["g++", "-x", "c++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "t2.o")])
    subprocess.check_call([str(tmp_path / "t")])


def test_argument_errors():
    """refused before any device is touched"""
    import libdwt_amd as dwt

    n, lines, levels = 32, 3, 4
    x = np.zeros((lines, n), F32)
    h = np.zeros((levels, lines, n), F32)
    l = np.zeros((levels, lines, n), F32)
    fv = np.zeros((lines, 2 * levels), F32)
    ls, ps = n * 4, lines * n * 4
    bad = [
        lambda: dwt.swt1d_batch("cdf53_i", x, ls, 4, lines, n, levels, h, None, 0, ps, ls),  # bad wavelet
        lambda: dwt.swt1d_batch(7, x, ls, 4, lines, n, levels, h, None, 0, ps, ls),
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, -1, h, None, 0, ps, ls),  # negative levels
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, 25, h, None, 0, ps, ls),  # above the cap
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, h, None, 2, ps, ls),  # l_mode 2 without dst_l
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, h, l, 3, ps, ls),
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, x, None, 0, ps, ls),  # dst_h is src
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, h, x.ctypes.data + 8, 1, ps, ls),  # dst_l inside src
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, h, h.ctypes.data + ps, 1, ps, ls),  # dst_l inside dst_h
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, h, l, 2, ps - 4, ls),  # planes overlap
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 4, lines, n, levels, h, l, 2, ps, ls - 4),  # lines overlap
        lambda: dwt.swt1d_batch("cdf97_s", x, ls, 2, lines, n, levels, h, l, 2, ps, ls),  # element stride
        lambda: dwt.swt_features1d_batch("cdf53_d", "wps", x, ls, 4, lines, n, levels, fv, 2 * levels),
        lambda: dwt.swt_features1d_batch("cdf53_s", "wps", x, ls, 4, lines, n, -2, fv, 2 * levels),
        lambda: dwt.swt_features1d_batch("cdf53_s", "wps", x, ls, 4, lines, n, 25, fv, 2 * levels),
        lambda: dwt.swt_features1d_batch("cdf53_s", ["wps", "med"], x, ls, 4, lines, n, levels, fv, 2 * levels - 1),  # fv stride
        lambda: dwt.swt_features1d_batch("cdf53_s", 0, x, ls, 4, lines, n, levels, fv, 2 * levels),  # empty mask
        lambda: dwt.swt_features1d_batch("cdf53_s", "wps", x, ls, 4, lines, n, levels, fv, 2 * levels, band=2),
        lambda: dwt.swt_features1d_batch("cdf53_s", "lpnorm", x, ls, 4, lines, n, levels, fv, 2 * levels, p=0.0),
        lambda: dwt.swt_cdf97_f_ex_stride_s(x, l, h, n, 4, 24),
        lambda: dwt.swt_cdf53_f_ex_stride_s(x, l, h, n, 4, -1),
        lambda: dwt.swt_cdf53_f_ex_stride_s(x, l, h, n, 2, 0),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    # the same refusals at the C-ABI, which the Python checks above stand in front of
    lib = dwt.lib
    assert lib.dwt_hip_swt1d_batch(1, x.ctypes.data, ls, 4, lines, n, levels, h.ctypes.data, None, 0, ps, ls) != 0
    assert lib.dwt_hip_swt1d_batch(0, x.ctypes.data, ls, 4, lines, n, 25, h.ctypes.data, None, 0, ps, ls) != 0
    assert lib.dwt_hip_swt1d_batch(0, x.ctypes.data, ls, 4, lines, n, -1, h.ctypes.data, None, 0, ps, ls) != 0
    assert lib.dwt_hip_swt1d_batch(0, x.ctypes.data, ls, 4, lines, n, levels, h.ctypes.data, l.ctypes.data, 5, ps, ls) != 0
    assert lib.dwt_hip_swt1d_level(0, x.ctypes.data, l.ctypes.data, h.ctypes.data, n, 4, 24) != 0
    assert lib.dwt_hip_swt_features1d_batch(0, 1, x.ctypes.data, ls, 4, lines, n, 25, 0, 2.0, fv.ctypes.data, 2 * levels) != 0
    assert lib.dwt_hip_swt_features1d_batch(0, 1, x.ctypes.data, ls, 4, lines, n, levels, 2, 2.0, fv.ctypes.data, 2 * levels) != 0
    assert b"SWT" in lib.dwt_hip_last_error()


def test_call_with_or_without_device():
    """without a device every call fails cleanly (DwtError, no abort); with one, a small call gives the restatement"""
    import libdwt_amd as dwt

    n, levels = 40, 3
    x = sm.make_input(5, "normal", 2, n)
    h = np.zeros((levels, 2, n), F32)
    l = np.zeros((1, 2, n), F32)
    fv = np.zeros((2, levels), F32)
    l1, h1 = np.zeros(n, F32), np.zeros(n, F32)
    calls = [
        lambda: dwt.swt1d_batch("cdf97_s", x, n * 4, 4, 2, n, levels, h, l, 1, 2 * n * 4, n * 4),
        lambda: dwt.swt_features1d_batch("cdf97_s", "wps", x, n * 4, 4, 2, n, levels, fv, levels),
        lambda: dwt.swt_cdf53_f_ex_stride_s(x[0], l1, h1, n, 4, 1),
    ]
    if dwt.lib.dwt_hip_init() != 0:
        for f in calls:
            with pytest.raises(dwt.DwtError) as e:
                f()
            assert "device" in str(e.value)
        return
    for f in calls:
        f()
    L, H = sm.swt_levels(x, "cdf97_s", levels)
    assert sm.same(h, H) and sm.same(l[0], L[-1])
    L1, H1 = sm.swt_level(x[0], "cdf53_s", 1)
    assert sm.same(l1, L1) and sm.same(h1, H1)
