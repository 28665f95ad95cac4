"""GPU parity of every float entry on the two input classes of tests/floatends.py, which the CPU suite pins to the reference
(tests/test_float_ends.py, tests/golden/float_ends.npz): `finite` -- no NaN or Inf in any result, so `same_floats` is plain
bit equality over every sample -- and `ends` -- finite values above MAX/2 next to the line ends, NaN share of a result at
most 0.25, and per (entry, direction) samples that a kernel with reflected ends c*(x+x) instead of the reference's (2c)*x
gets wrong.  An inverse runs on the input itself, read as coefficients.  These classes carry the line-end claim of the
README, inverses included; tests/test_hip_float_range.py keeps the whole range.

One row of ROUTES per entry: how the case's forward and inverse reach the library.  The 3-D entries are compared with the
oracle's reflected-ends form (their listed difference); under DWT_HIP_LIB=...libdwt_hip_plain... (reflected
ends in every float kernel) everything is, as in tests/test_hip_float_range.py."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import floatends as F
from conftest import GOLDEN, bits, same_floats
from test_float_ends import float_ends_cases, float_ends_input

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=RuntimeWarning)

PLAIN_BUILD = os.path.basename(os.environ.get("DWT_HIP_LIB", "")).startswith("libdwt_hip_plain")
WID = {"cdf97": 0, "cdf53": 2, "interp53": 6}  # DWT_HIP_CDF97_S, DWT_HIP_CDF53_S, DWT_HIP_INTERP53_S


@pytest.fixture(scope="module")
def dwt():
    import libdwt_amd as d

    d.dwt_util_init()
    d.poison_workspace(0xFFFFFFFF)  # every call below starts on scratch that holds NaN / -1 in every word
    yield d
    d.poison_workspace(None)
    for k, v in (("fma", 0), ("vol_fused", 1), ("vol_tile_pairs", 0), ("generic", 0)):
        d.set_option(k, v)
    d.dwt_util_set_accel(0)
    d.dwt_util_finish()


@pytest.fixture(scope="module")
def stored():
    return np.load(os.path.join(GOLDEN, "float_ends.npz"))


def reflected(e):
    return PLAIN_BUILD or e == "cdf97_3d"


def expected(oracle, m, a):
    """(forward of a, inverse of a) the kernels must produce for fixture case `m`."""
    e, d1 = m["entry"], m["decompose_one"]
    with (F.reflected_ends(oracle) if reflected(e) else warnings.catch_warnings()):
        fwd, j = F.transform(oracle, e, 0, a, m["j_in"], d1)
        assert j == m["j_out"]
        inv, _ = F.transform(oracle, e, 1, a, j, d1)
    return fwd, inv


# ---- the routes: (dwt, m, a, inverse) -> the result ----------------------------------------------------------------------
def _entry2d(dwt, e, inverse):
    if e.endswith("_il"):
        return getattr(dwt, "dwt_%s_%s_inplace_s" % (e[:5], "2i" if inverse else "2f"))
    if e == "interp53_2d":
        return dwt.dwt_interp53_2i_s if inverse else dwt.dwt_interp53_2f_s
    return (dwt.INVERSE if inverse else dwt.FORWARD)[e]


def host(dwt, m, a, inverse, accel=0):
    """The libdwt.h host-pointer entry, in place."""
    h, w = a.shape
    got = a.copy()
    dwt.dwt_util_set_accel(accel)
    try:
        j = _entry2d(dwt, m["entry"], inverse)(got, got.strides[0], a.itemsize, w, h, w, h, m["j_out"] if inverse else m["j_in"],
                                               m["decompose_one"])
    finally:
        dwt.dwt_util_set_accel(0)
    assert inverse or j == m["j_out"]
    return got


def host_line_passes(dwt, m, a, inverse):
    return host(dwt, m, a, inverse, accel=1)


def device(dwt, m, a, inverse):
    """The same entry on a device-resident image, in place (Mallat: staged, the copy riding along)."""
    h, w = a.shape
    d = dwt.DeviceImage(h, w, itemsize=a.itemsize).upload(a)
    try:
        _entry2d(dwt, m["entry"], inverse)(d.ptr, d.stride_x, a.itemsize, w, h, w, h, m["j_out"] if inverse else m["j_in"], m["decompose_one"])
        return d.download(a.dtype)
    finally:
        d.free()


def device_s2(dwt, m, a, inverse):
    """dwt_cdf97_2f_s2 / _2i_s2 and the interleaved entries out of place: device images, the source left as it was."""
    h, w = a.shape
    e = m["entry"]
    src, dst = dwt.DeviceImage(h, w).upload(a), dwt.DeviceImage(h, w).upload(np.full_like(a, 7.0))
    try:
        j = m["j_out"] if inverse else m["j_in"]
        if e.endswith("_il"):
            dwt.transform2d_interleaved(e[:5] + "_s", inverse, 0, src.ptr, dst.ptr, src.stride_x, 4, w, h, None, None, j, m["decompose_one"])
        else:
            (dwt.dwt_cdf97_2i_s2 if inverse else dwt.dwt_cdf97_2f_s2)(src.ptr, dst.ptr, dst.stride_x, 4, w, h, w, h, j, m["decompose_one"])
        assert np.array_equal(bits(src.download(a.dtype)), bits(a)), "source image modified"
        return dst.download(a.dtype)
    finally:
        src.free()
        dst.free()


def line_batch(dwt, m, a, inverse):
    """dwt_hip_transform1d_batch on device rows: one launch up to 8192 samples; longer lines (8197, 8200) take their
    leading levels pass by pass."""
    n_lines, n = a.shape
    d = dwt.DeviceImage(n_lines, n).upload(a)
    try:
        jj = C.c_int(m["j_out"] if inverse else m["j_in"])
        n0 = dwt.get_option("stat_launches")
        rc = dwt.lib.dwt_hip_transform1d_batch(WID[m["entry"][:-3]], inverse, d.ptr, d.ptr, n * 4, 4, n_lines, n, n, C.byref(jj), 0)
        assert rc == 0, dwt.last_error()
        if n <= 8192:
            assert dwt.get_option("stat_launches") - n0 == 1, "the one-launch route"
        return d.download(np.float32)
    finally:
        d.free()


def host_lines(dwt, m, a, inverse):
    """The libdwt.h 1-D host entries, line by line."""
    got = a.copy()
    fn = getattr(dwt, "dwt_%s_%s_s" % (m["entry"][:-3], "1i" if inverse else "1f"))
    for y in range(got.shape[0]):
        fn(got[y], 4, got.shape[1], got.shape[1], m["j_out"] if inverse else m["j_in"])
    return got


def _vol(dwt, m, v, inverse, mode):
    nz, ny, nx = v.shape
    src, dst = dwt.lib.dwt_hip_malloc(v.nbytes), dwt.lib.dwt_hip_malloc(v.nbytes)
    got = np.empty_like(v)
    try:
        assert src and dst and dwt.lib.dwt_hip_memcpy_h2d(src, v.ctypes.data, v.nbytes) == 0
        if mode == "op":
            dwt.transform3d_op(src, dst, nx * 4, nx * ny * 4, nx, ny, nz, 1)
            assert dwt.lib.dwt_hip_memcpy_d2h(got.ctypes.data, dst, v.nbytes) == 0
            return got
        if mode == "ip-fused":
            dwt.set_option("vol_fused", 2)
            dwt.set_option("vol_tile_pairs", 8)
        dwt.transform3d(inverse, src, nx * 4, nx * ny * 4, nx, ny, nz, 1)
        assert dwt.lib.dwt_hip_memcpy_d2h(got.ctypes.data, src, v.nbytes) == 0
        return got
    finally:
        dwt.set_option("vol_fused", 1)
        dwt.set_option("vol_tile_pairs", 0)
        dwt.lib.dwt_hip_free(src)
        dwt.lib.dwt_hip_free(dst)


def vol_op(dwt, m, v, inverse):
    """One 3-D level out of place (forward only: the fused x+y+z kernel where the volume is wide enough)."""
    return None if inverse else _vol(dwt, m, v, 0, "op")


def vol_ip(dwt, m, v, inverse):
    return _vol(dwt, m, v, inverse, "ip")


def vol_ip_fused(dwt, m, v, inverse):
    """In place through the one-pass level over the halo snapshot (rows of 256 samples and more)."""
    return None if v.shape[2] < 256 else _vol(dwt, m, v, inverse, "ip-fused")


MALLAT = [host, host_line_passes, device]
ROUTES = {
    "cdf97_s": MALLAT + [device_s2],
    "cdf53_s": MALLAT,
    "cdf97_d": MALLAT,
    "cdf53_d": MALLAT,
    "cdf97_il": MALLAT + [device_s2],
    "cdf53_il": MALLAT + [device_s2],
    "cdf97_1d": [line_batch, host_lines],
    "cdf53_1d": [line_batch, host_lines],
    "interp53_2d": MALLAT,
    "interp53_1d": [line_batch, host_lines],
    "cdf97_3d": [vol_op, vol_ip, vol_ip_fused],
}
assert set(ROUTES) == set(F.ENTRIES)
PARAMS = [pytest.param(m, r, id="%s-%s" % (m["name"], r.__name__)) for m in float_ends_cases() for r in ROUTES[m["entry"]]]


@pytest.mark.parametrize("m,route", PARAMS)
def test_entry_on_the_finite_and_ends_classes(dwt, oracle, stored, m, route):
    """Forward and inverse of the case through one route, each against the oracle under `same_floats`; on the finite class
    that is every bit.  Cases stored in full are the reference's own outputs."""
    a = float_ends_input(m)
    want = expected(oracle, m, a)
    for inverse in (0, 1):
        got = route(dwt, m, a, inverse)
        if got is None:
            continue  # (the route has no such direction, or not at this size)
        what = (m["name"], route.__name__, "inverse" if inverse else "forward", F.telling(got, want[inverse]))
        assert same_floats(got, want[inverse]), what
        if m["klass"] == "finite":
            assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want[inverse])), what
        if m["full"] and not reflected(m["entry"]):
            assert same_floats(got, stored[m["name"] + (".inv" if inverse else ".fwd")]), what


@pytest.mark.parametrize("m", [m for m in float_ends_cases() if m["entry"] == "cdf97_s" and m["klass"] == "finite"], ids=lambda m: m["name"])
def test_fma_option_on_the_finite_class(dwt, oracle, m):
    """Option `fma` contracts each lifting step: not the reference's rounding, held to 1e-5 of the largest coefficient as
    in tests/test_hip_float_range.py -- on the finite class, where every sample counts; host and device entries."""
    a = float_ends_input(m)
    want = expected(oracle, m, a)
    dwt.set_option("fma", 1)
    try:
        for route in (host, device, device_s2):
            for inverse in (0, 1):
                got = route(dwt, m, a, inverse)
                assert np.isfinite(got).all()
                g, w_ = got.astype(np.float64), want[inverse].astype(np.float64)
                scale = max(np.abs(w_).max(), float(np.finfo(np.float32).tiny))
                assert np.abs(g - w_).max() <= 1e-5 * scale, (route.__name__, inverse)
    finally:
        dwt.set_option("fma", 0)
