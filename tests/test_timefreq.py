"""CPU checks of the time-frequency planes: the numpy float32 restatement (tests/timefreq_model.py) against the reference's
outputs (tests/golden/timefreq.npz, written by scripts/gen_timefreq_golden.py), the kernel generators of the built library
(host code) against the reference's kernels, the ABI, the argument checks, and a call without a device."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import timefreq_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(tm.GOLDEN)
with open(tm.MANIFEST) as _f:
    INFO = json.load(_f)
F32 = np.float32
IDS = ["-".join(str(v) for v in c) for c in tm.CASES]


def bank_of(i):
    sizes, centers = GOLD["sizes_%d" % i], GOLD["centers_%d" % i]
    return sizes, centers, np.split(GOLD["taps_%d" % i], np.cumsum(sizes)[:-1])


def test_manifest():
    info = INFO["files"]["timefreq.npz"]
    with open(tm.GOLDEN, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == info["sha256"]
    assert [(c["seed"], c["kind"], c["input"], c["n"], c["bins"], c["sigma"], c["freq"]) for c in info["cases"]] == tm.CASES
    assert os.path.getsize(tm.GOLDEN) < 1 << 20
    assert os.path.getsize(tm.GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                                             if f != "timefreq.npz")
    assert {c[3] for c in tm.CASES} == {1, 2, 7, 64, 333, 1024} and {c[4] for c in tm.CASES} == {1, 5, 16, 64}
    assert {c[1] for c in tm.CASES} == {"ft", "wt", "st"} and "float_range" in {c[2] for c in tm.CASES}
    assert any(GOLD["sizes_%d" % i].max() > c[3] for i, c in enumerate(tm.CASES))  # kernels longer than the signal
    # no point of the committed planes is excused from the detect_ridges3_s comparison
    assert INFO["ridges3_excluded_points"] == 0 and INFO["ridges3_min_margin"] > 2.0 ** -20


@pytest.mark.parametrize("i", range(len(tm.CASES)), ids=IDS)
def test_restatement_equals_golden(i):
    x = GOLD["x_%d" % i]
    assert tm.same(x, tm.make_input(tm.CASES[i][0], tm.CASES[i][2], 1, tm.CASES[i][3])[0])
    re, im, mag = tm.planes(x, *bank_of(i))
    dots = GOLD["dots_%d" % i]
    assert tm.same(re, dots[..., 0]) and tm.same(im, dots[..., 1])
    assert tm.same(mag, GOLD["mag_%d" % i])
    pd = tm.phase_derivative(GOLD["arg_%d" % i], INFO["phase_limit"])
    assert tm.same(pd, GOLD["pd_%d" % i])
    assert tm.same(tm.ridges1(GOLD["mag_%d" % i], 0.0), GOLD["r1_%d" % i])
    assert tm.same(tm.ridges2(GOLD["pd_%d" % i], 0.0), GOLD["r2_%d" % i])
    assert tm.ridges3_margin(GOLD["mag_%d" % i]) > 2.0 ** -20


def test_reference_arg_error_is_what_the_manifest_says():
    worst = 0.0
    for i in range(len(tm.CASES)):
        d = GOLD["dots_%d" % i].astype(np.float64)
        with np.errstate(all="ignore"):
            e = tm.ulps(GOLD["arg_%d" % i], np.arctan2(d[..., 1], d[..., 0]))
        worst = max(worst, float(e[np.isfinite(e)].max()))
    assert worst == INFO["arg_ref_max_ulp"] and worst < 4


@pytest.mark.parametrize("i", range(len(tm.CASES)), ids=IDS)
def test_bank_generators(i):
    """the library's generators (host code): sizes and centres exactly; the taps within the manifest's observed maximum
    plus 1 ulp -- a measured margin for another host libm: two faithful expf / sincosf may round to neighbouring floats"""
    import libdwt_amd as dwt

    _, kind, _, _, bins, sigma, freq = tm.CASES[i]
    bank = dwt.timefreq_bank(kind, bins, sigma, freq)
    sizes, centers, taps = bank.query()
    bank.free()
    want_s, want_c, want_t = bank_of(i)
    assert np.array_equal(sizes, want_s) and np.array_equal(centers, want_c)
    worst = 0.0
    for y in range(bins):
        for part in (np.real, np.imag):
            worst = max(worst, float(tm.ulps(part(taps[y]), part(want_t[y]).astype(np.float64)).max()))
    print("largest tap difference: %g ulp" % worst)
    assert worst <= INFO["tap_max_ulp"] + 1
    # a bank of the caller's kernels gives them back
    bank = dwt.timefreq_bank(kernels=want_t, centers=want_c)
    s2, c2, t2 = bank.query()
    bank.free()
    assert np.array_equal(s2, want_s) and np.array_equal(c2, want_c) and all(tm.same(a.view(F32), b.view(F32)) for a, b in zip(t2, want_t))


def test_generator_entries():
    import libdwt_amd as dwt

    assert dwt.lib.dwt_hip_gaussian_size(40.0, 1.0) == 321 and dwt.lib.dwt_hip_gaussian_size(1.0, 0.999) == 9
    bank = dwt.timefreq_bank("wt", 256, 1.0, tm.FREQ_TF)  # the spectra-tf settings: ceilf(1 + 8 * 0.999 * 256) = 2047 taps down to 9
    sizes, _, _ = bank.query()
    assert sizes.min() == 9 and sizes.max() == 2047
    bank.free()
    bank = dwt.timefreq_bank("st", 256)
    assert bank.query()[0].max() == 2898  # ceilf(1 + 8 * sqrtf(1 / 2) * 512)
    bank.free()


NEW_SYMBOLS = ["dwt_hip_timefreq_bank_create", "dwt_hip_timefreq_bank_from_kernels", "dwt_hip_timefreq_bank_free", "dwt_hip_timefreq_bank_bins",
               "dwt_hip_timefreq_bank_taps", "dwt_hip_timefreq_bank_query", "dwt_hip_timefreq_batch", "dwt_hip_timefreq_batch_strided",
               "dwt_hip_cdot1", "dwt_hip_phase_derivative", "dwt_hip_detect_ridges", "dwt_hip_gabor_transform", "dwt_hip_timefreq_line",
               "dwt_hip_gaussian_size", "dwt_hip_gabor_wavelet", "dwt_hip_gabor_gen_kernel", "dwt_util_cdot1_s"]


def test_abi_exports():
    lib = C.CDLL(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so"))
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    import libdwt_amd as dwt

    for s in ["timefreq_bank", "timefreq_batch", "gabor_ft_s", "gabor_wt_s", "gabor_st_s", "gabor_ft_arg_s", "gabor_wt_arg_s", "gabor_st_arg_s",
              "phase_derivative", "detect_ridges"]:
        assert callable(getattr(dwt, s)), s
    assert dwt.lib.dwt_hip_get_option(b"timefreq_tiled") == 1


def test_gabor_header_compiles_and_links(tmp_path):
    """include/gabor.h gives the reference's prototypes: a caller written against src/gabor.h compiles (C99 and C++) and
    links against the library with nothing but the header; the generators run without a device"""
    src = tmp_path / "t.c"
    src.write_text('#include "gabor.h"\n#include <stdio.h>\nint main(int argc, char **argv){float x[8]={0},p[32];float _Complex *k=0;(void)argv;'
                   'gabor_gen_kernel(&k,sizeof(float _Complex),2.f,1.f,1.f);printf("%d %d %.9g %.9g\\n",gaussian_size(2.f,1.f),gaussian_center(2.f,1.f),'
                   '(double)__real__ k[8],(double)__real__ gabor_function(0.f,2.f,1.f));free(k);if(argc>99){gabor_ft_s(x,4,8,p,32,4,4,1.f);gabor_ft_arg_s(x,4,8,p,32,4,4,1.f);'
                   'gabor_wt_s(x,4,8,p,32,4,4,1.f,3.f);gabor_wt_arg_s(x,4,8,p,32,4,4,1.f,3.f);gabor_st_s(x,4,8,p,32,4,4);gabor_st_arg_s(x,4,8,p,32,4,4);'
                   'timefreq_line(p,4,x,4,8,k,8,17,8);timefreq_arg_line(p,4,x,4,8,k,8,17,8);(void)dwt_util_cdot1_s(x,8,4,0,k,17,8,8);'
                   'phase_derivative_s(p,p+16,16,4,4,4,3.f);detect_ridges1_s(p,p+16,16,4,4,4,0.f);detect_ridges2_s(p,p+16,16,4,4,4,0.f);'
                   'detect_ridges3_s(p,p+16,16,4,4,4,0.f);}return 0;}\n')
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "libdwt_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-l:libdwt_hip.so", "-Wl,-rpath," + libdir])
    subprocess.check_call(["g++", "-x", "c++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "t2.o")])
    out = subprocess.check_output([str(tmp_path / "t")]).decode().split()
    alpha = F32(F32(F32(1) / F32(2)) / F32(2)) / F32(2)
    centre = F32(np.sqrt(F32(alpha / tm.PI)))  # the tap at the centre: sqrtf(alpha / pi) * expf(0) * cexpf(0)
    assert out[:2] == ["17", "8"] and F32(float(out[2])) == centre and F32(float(out[3])) == centre


def test_argument_errors():
    """refused before any device is touched"""
    import libdwt_amd as dwt

    n, lines, bins = 32, 3, 4
    x = np.zeros((lines, n), F32)
    out = np.zeros((lines, bins, n), F32)
    ls, rs, ps = n * 4, n * 4, bins * n * 4
    bank = dwt.timefreq_bank("st", bins)
    bad = [
        lambda: dwt.timefreq_bank("xx", bins),
        lambda: dwt.timefreq_bank("ft", 0, 1.0),  # bins
        lambda: dwt.timefreq_bank("ft", bins, 0.0),  # sigma
        lambda: dwt.timefreq_bank("wt", bins, 1.0, 0.0),  # frequency
        lambda: dwt.timefreq_bank("ft", bins, float("nan")),
        lambda: dwt.timefreq_bank("ft", bins, 1e30),  # a size no int holds
        lambda: dwt.timefreq_bank(kernels=[np.zeros(3, np.complex64)], centers=[3]),  # centre outside the kernel
        lambda: dwt.timefreq_bank(kernels=[np.zeros(0, np.complex64)], centers=[0]),
        lambda: dwt.timefreq_batch(bank, x, ls, 4, lines, n, "power", out, ps, rs),
        lambda: dwt.timefreq_batch(bank, x, ls, 4, 0, n, "abs", out, ps, rs),  # no line
        lambda: dwt.timefreq_batch(bank, x, ls, 4, lines, 0, "abs", out, ps, rs),  # no sample
        lambda: dwt.timefreq_batch(bank, x, ls, 2, lines, n, "abs", out, ps, rs),  # element stride
        lambda: dwt.timefreq_batch(bank, x, ls - 4, 4, lines, n, "abs", out, ps, rs),  # lines overlap
        lambda: dwt.timefreq_batch(bank, x, ls, 4, lines, n, "abs", out, ps, rs - 4),  # rows overlap
        lambda: dwt.timefreq_batch(bank, x, ls, 4, lines, n, "abs", out, ps - 4, rs),  # planes overlap
        lambda: dwt.timefreq_batch(bank, x, ls, 4, lines, n, "complex", out, ps, rs),  # rows of complex pairs overlap
        lambda: dwt.timefreq_batch(bank, x, ls, 4, lines, n, "abs", x, ps, rs),  # dst is src
        lambda: dwt.timefreq_batch(bank, out, ls, 4, lines, n, "abs", out.ctypes.data + 64, ps, rs),  # dst inside src
        lambda: dwt.phase_derivative(out, out, rs, 4, n, bins, 3.0),  # in place
        lambda: dwt.phase_derivative(out[0], out[1], rs, 4, n, bins, 0.0),  # limit
        lambda: dwt.phase_derivative(out[0], out[1], rs, 4, 0, bins, 3.0),
        lambda: dwt.phase_derivative(out[0], out[2], rs, 4, n, bins, 3.0, 2, ps - 4),  # planes overlap
        lambda: dwt.detect_ridges(0, out[0], out[1], rs, 4, n, bins, 0.0),
        lambda: dwt.detect_ridges(4, out[0], out[1], rs, 4, n, bins, 0.0),
        lambda: dwt.detect_ridges(1, out[0], out[1], rs - 4, 4, n, bins, 0.0),  # rows overlap
        lambda: dwt.detect_ridges(1, out[0], out[1], rs, 2, n, bins, 0.0),
        lambda: dwt.gabor_ft_s(x, 4, n, out, rs, 4, bins, -1.0),
        lambda: dwt.gabor_wt_s(x, 4, n, out, rs, 4, bins, 1.0, 0.0),
        lambda: dwt.gabor_st_s(x, 4, 0, out, rs, 4, bins),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(dwt.DwtError) as e:
            f()
        assert len(str(e.value)) > 10, i
    bank.free()
    with pytest.raises(dwt.DwtError):
        dwt.timefreq_batch(bank, x, ls, 4, lines, n, "abs", out, ps, rs)  # a freed bank
    lib = dwt.lib
    assert lib.dwt_hip_timefreq_batch(None, x.ctypes.data, ls, 4, lines, n, 1, out.ctypes.data, ps, rs) != 0
    assert b"bank" in lib.dwt_hip_last_error()
    assert lib.dwt_hip_timefreq_bank_create(3, 4, 1.0, 1.0) is None and lib.dwt_hip_timefreq_bank_from_kernels(0, None, None, None) is None
    assert lib.dwt_hip_cdot1(x.ctypes.data, n, 4, n, out.ctypes.data, 4, 8, 2, out.ctypes.data) != 0  # centre outside the signal


def test_call_with_or_without_device():
    """without a device every call fails cleanly (DwtError, no abort); with one, a small call gives the fixture"""
    import libdwt_amd as dwt

    i = 3
    _, kind, _, n, bins, sigma, freq = tm.CASES[i]
    x = GOLD["x_%d" % i]
    mag, pd = np.zeros((bins, n), F32), np.zeros((bins, n), F32)
    bank = dwt.timefreq_bank(kernels=bank_of(i)[2], centers=bank_of(i)[1])
    calls = [
        lambda: dwt.timefreq_batch(bank, x, n * 4, 4, 1, n, "abs", mag, bins * n * 4, n * 4),
        lambda: dwt.phase_derivative(GOLD["arg_%d" % i], pd, n * 4, 4, n, bins, INFO["phase_limit"]),
        lambda: dwt.detect_ridges(1, GOLD["mag_%d" % i], pd, n * 4, 4, n, bins, 0.0),
    ]
    if dwt.lib.dwt_hip_init() != 0:
        for f in calls:
            with pytest.raises(dwt.DwtError) as e:
                f()
            assert "device" in str(e.value)
        return
    for f in calls:
        f()
    assert tm.same(mag, GOLD["mag_%d" % i]) and tm.same(pd, GOLD["r1_%d" % i])
