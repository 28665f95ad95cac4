"""CPU checks of the 1-D entries (dwt_cdf{97,53}_1f_s / _1i_s / _2f1_s): the header declares them with the
reference's own types, the library exports them, and the test-side restatement of the 1-D driver -- the oracle's line
functions composed level by level, as the reference's loop composes its line kernels (src/libdwt.c:15766-16130) -- is
pinned to the compiled reference.  tests/test_hip_oned.py holds the GPU path to the same restatement / reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES_1D = ["dwt_cdf97_1f_s", "dwt_cdf53_1f_s", "dwt_cdf97_1i_s", "dwt_cdf53_1i_s", "dwt_cdf97_2f1_s", "dwt_cdf53_2f1_s"]
J_CASES = [-1, 0, 1, 2, 3, 99]

_I, _P = C.c_int, C.c_void_p


def cdp2(n, j):
    return (n + (1 << j) - 1) >> j


def ceil_log2(x):
    n = 0
    while n < 31 and (1 << n) < x:
        n += 1
    return n


def restated(oracle, wv, inverse, a, so, si=None, j_max=-1, zero_padding=0):
    """The reference's 1-D driver on the float32 line `a` (its first `so` samples are the frame), in place, from the
    oracle's exact line transforms.  Returns the level count (forward: as stored in *j_max_ptr)."""
    si = so if si is None else si
    j_limit = ceil_log2(so)
    if not inverse:
        J = j_limit if (j_max < 0 or j_max > j_limit) else j_max
        for j in range(J):
            so_src, so_dst, si_src = cdp2(so, j), cdp2(so, j + 1), cdp2(si, j)
            nl, nh = (si_src + 1) // 2, si_src // 2
            if so_src > 1:
                t = a[:si_src].copy()
                oracle.line("%s_f_s" % wv, t)
                a[:nl] = t[0::2]
                a[so_dst:so_dst + nh] = t[1::2]
            if zero_padding:
                a[nl:so_dst] = 0
                a[so_dst + nh:so_src] = 0
        return J
    J = j_limit
    if 0 <= j_max < J:
        J = j_max
    for j in range(J, 0, -1):
        so_src, so_dst, si_dst = cdp2(so, j), cdp2(so, j - 1), cdp2(si, j - 1)
        if so_dst > 1:
            n = si_dst
            t = np.empty(n, np.float32)
            t[0::2] = a[:(n + 1) // 2]
            t[1::2] = a[so_src:so_src + n // 2]
            oracle.line("%s_i_s" % wv, t)
            a[:n] = t
        if zero_padding:
            a[si_dst:so_dst] = 0
    return j_max


def ref_lib(reference):
    """The reference's 1-D entries with their ctypes signatures."""
    L = reference.lib
    for wv in ("cdf97", "cdf53"):
        getattr(L, "dwt_%s_1f_s" % wv).argtypes = [_P, _I, _I, _I, C.POINTER(_I), _I]
        getattr(L, "dwt_%s_1i_s" % wv).argtypes = [_P, _I, _I, _I, _I, _I]
        getattr(L, "dwt_%s_2f1_s" % wv).argtypes = [_P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I]
        for k in ("1f", "1i", "2f1"):
            getattr(L, "dwt_%s_%s_s" % (wv, k)).restype = None
    return L


def ref_call(L, wv, inverse, a, so, si=None, j_max=-1, zero_padding=0, stride=4):
    """The compiled reference on the buffer of `a` (in place).  Returns *j_max_ptr (forward) or j_max."""
    si = so if si is None else si
    if not inverse:
        j = _I(j_max)
        getattr(L, "dwt_%s_1f_s" % wv)(a.ctypes.data, stride, so, si, C.byref(j), zero_padding)
        return j.value
    getattr(L, "dwt_%s_1i_s" % wv)(a.ctypes.data, stride, so, si, j_max, zero_padding)
    return j_max


@pytest.fixture(scope="module")
def dwt():
    import __graft_entry__ as g

    if not os.path.exists(os.path.join(ROOT, "libdwt_amd", "libdwt_hip.so")):
        g.build()
    import libdwt_amd

    return libdwt_amd


def test_header_declares_the_reference_types(tmp_path):
    """A C99 unit that assigns each entry to a pointer of the reference's type (as examples/function-iterating does):
    any difference in a parameter type is a compile error."""
    src = tmp_path / "types.c"
    src.write_text("""#include "libdwt.h"
typedef void (*fwd1_t)(void *, int, int, int, int *, int);
typedef void (*inv1_t)(void *, int, int, int, int, int);
typedef void (*ser_t)(void *, int, int, int, int, int, int, int *, int);
fwd1_t f1[] = { dwt_cdf97_1f_s, dwt_cdf53_1f_s };
inv1_t i1[] = { dwt_cdf97_1i_s, dwt_cdf53_1i_s };
ser_t s1[] = { dwt_cdf97_2f1_s, dwt_cdf53_2f1_s };
""")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-o", str(tmp_path / "t.o"),
                        "-I", os.path.join(ROOT, "include")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_1d_entries(dwt):
    for name in ENTRIES_1D + ["dwt_hip_transform1d", "dwt_hip_transform1d_batch"]:
        assert hasattr(dwt.lib, name), name


def test_transform1d_fails_loudly_without_gpu(dwt):
    if dwt.device_count() > 0:
        pytest.skip("a GPU is present")
    a = np.zeros(64, np.float32)
    with pytest.raises(dwt.DwtError):
        dwt.transform1d_batch("cdf97_s", 0, a, a, 256, 1, 64)
    with pytest.raises(dwt.DwtError):
        dwt.dwt_cdf53_1f_s(a, 4, 64, 64)
    assert not a.any()


def test_transform1d_rejects_other_wavelets(dwt):
    a = np.zeros(64, np.float32)
    j = _I(-1)
    assert dwt.lib.dwt_hip_transform1d(1, 0, a.ctypes.data, a.ctypes.data, 4, 64, 64, C.byref(j), 0) != 0
    assert not a.any()


LENGTHS = list(range(1, 71)) + [127, 128, 129, 1000, 4095, 4096, 4097]


@pytest.mark.parametrize("wv", ["cdf97", "cdf53"])
@pytest.mark.parametrize("inverse", [0, 1], ids=["fwd", "inv"])
def test_restatement_matches_reference(oracle, reference, wv, inverse):
    L = ref_lib(reference)
    rng = np.random.default_rng(11 + inverse)
    for n in LENGTHS:
        for j in J_CASES:
            a = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
            want, got = a.copy(), a.copy()
            jw = ref_call(L, wv, inverse, want, n, j_max=j)
            jg = restated(oracle, wv, inverse, got, n, j_max=j)
            assert jw == jg and np.array_equal(want.view(np.uint32), got.view(np.uint32)), (wv, inverse, n, j)


@pytest.mark.parametrize("wv", ["cdf97", "cdf53"])
def test_restatement_matches_reference_sparse(oracle, reference, wv):
    """size_o > size_i, with and without zero padding, forward and inverse (a strided line: elements 8 bytes apart)."""
    L = ref_lib(reference)
    rng = np.random.default_rng(5)
    for so, si in ((9, 5), (16, 13), (33, 1), (70, 0), (100, 61), (257, 200)):
        for zp in (0, 1):
            for inverse in (0, 1):
                for j in (-1, 2):
                    buf = (rng.random(2 * so, dtype=np.float32) - 0.5).astype(np.float32)
                    want = buf.copy()
                    jw = ref_call(L, wv, inverse, want, so, si, j, zp, stride=8)
                    got = buf.copy()
                    line = got[0::2].copy()
                    jg = restated(oracle, wv, inverse, line, so, si, j, zp)
                    got[0::2] = line
                    assert jw == jg and np.array_equal(want.view(np.uint32), got.view(np.uint32)), (wv, so, si, zp, inverse, j)


@pytest.mark.parametrize("wv", ["cdf97", "cdf53"])
def test_series_is_rowwise_forward(oracle, reference, wv):
    """_2f1_s: rows 0 .. size_i_big_y-1 of a padded matrix, each the 1-D forward; rows below and the padding untouched;
    *j_max_ptr clamped once (and untouched without rows)."""
    L = ref_lib(reference)
    rng = np.random.default_rng(3)
    h, w, pitch = 7, 37, 41
    m = np.full((h, pitch), 7.25, np.float32)
    m[:, :w] = rng.random((h, w), dtype=np.float32)
    want = m.copy()
    j = _I(99)
    getattr(L, "dwt_%s_2f1_s" % wv)(want.ctypes.data, pitch * 4, 4, w, h, w, 5, C.byref(j), 0)
    assert j.value == ceil_log2(w)
    got = m.copy()
    for y in range(5):
        line = got[y, :w].copy()
        restated(oracle, wv, 0, line, w, j_max=99)
        got[y, :w] = line
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    j = _I(-5)
    getattr(L, "dwt_%s_2f1_s" % wv)(want.ctypes.data, pitch * 4, 4, w, h, w, 0, C.byref(j), 0)
    assert j.value == -5
