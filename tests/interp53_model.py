"""A numpy restatement of libdwt's interpolating 5/3 wavelet -- CDF 5/3 with its predict step alone, no update step --
written from the reference's definition: the line transforms dwt_interp53_f_ex_stride_s / _i_ex_stride_s
(src/libdwt.c:11252-11291, 12004-12044; constants src/inline.h:332-335), the 2-D drivers dwt_interp53_2f_s / _2i_s
(:16801, :18457, those of dwt_cdf53_2f_s / _2i_s with the line function swapped) and the 1-D drivers
dwt_interp53_1f_s / _1i_s (:16166, :15900).  Every operation rounds to float32 as the reference's (FMA-free) build does,
so the results are the reference's bits over the whole float range.

`RefInterp53` calls the same four entries of the compiled reference (oracle/_ref/libdwt_ref.so) where it was built."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdwt_ref.so")

P1 = np.float32(0.5)
S1 = np.float32(1.41421356237309504880)
S2 = np.float32(0.70710678118654752440)
TWO_P1 = np.float32(2) * P1  # `2 * dwt_cdf53_p1_s`, a float
REFLECTED_ENDS = False  # True: the doubled tap as reflection gives it, p*(x+x) (tests/floatends.py counts against it)


def end2(x):
    """The two equal taps of the last odd sample of an even line: the reference's (2p)*x."""
    return P1 * (x + x) if REFLECTED_ENDS else TWO_P1 * x


def ceil_log2(x):
    j = 0
    while (1 << j) < x:
        j += 1
    return j


def ceil_div_pow2(x, j):
    return (x + (1 << j) - 1) >> j


# ---- one level over a batch of lines: t[line, sample] --------------------------------------------------------
def fwd_lines(t):
    """Forward lift and scale of the lines t (n_lines x N), in place on a copy; returns the interleaved result."""
    t = np.array(t, dtype=np.float32, copy=True)
    N = t.shape[1]
    if N < 2:
        if N == 1:
            t[:, 0] = t[:, 0] * S1
        return t
    odd = np.arange(1, N - 2 + (N & 1), 2)
    # the odd samples depend on the even ones only: the reference's loop order does not matter
    t[:, odd] = t[:, odd] - P1 * (t[:, odd - 1] + t[:, odd + 1])
    if N % 2 == 0:
        t[:, N - 1] = t[:, N - 1] - end2(t[:, N - 2])
    t[:, 0::2] = t[:, 0::2] * S1
    t[:, 1::2] = t[:, 1::2] * S2
    return t


def inv_lines(t):
    """Inverse of fwd_lines on interleaved lines (n_lines x N)."""
    t = np.array(t, dtype=np.float32, copy=True)
    N = t.shape[1]
    if N < 2:
        if N == 1:
            t[:, 0] = t[:, 0] * S2
        return t
    t[:, 0::2] = t[:, 0::2] * S2
    t[:, 1::2] = t[:, 1::2] * S1
    if N % 2 == 0:
        t[:, N - 1] = t[:, N - 1] + end2(t[:, N - 2])
    odd = np.arange(1, N - 2 + (N & 1), 2)
    t[:, odd] = t[:, odd] + P1 * (t[:, odd - 1] + t[:, odd + 1])
    return t


def _fwd_rows(a, n_rows, N, hoff):
    """dwt_interp53_f_ex_stride_s on rows 0 .. n_rows-1 of a: samples [0, N) -> L at [0, ceil(N/2)), H at hoff."""
    if N == 0 or n_rows == 0:
        return
    t = fwd_lines(a[:n_rows, :N])
    a[:n_rows, :(N + 1) // 2] = t[:, 0::2]
    a[:n_rows, hoff:hoff + N // 2] = t[:, 1::2]


def _inv_rows(a, n_rows, N, hoff):
    """dwt_interp53_i_ex_stride_s on rows 0 .. n_rows-1 of a: L at [0, ceil(N/2)), H at hoff -> samples [0, N)."""
    if N == 0 or n_rows == 0:
        return
    t = np.empty((n_rows, N), np.float32)
    t[:, 0::2] = a[:n_rows, :(N + 1) // 2]
    t[:, 1::2] = a[:n_rows, hoff:hoff + N // 2]
    a[:n_rows, :N] = inv_lines(t)


def _zero_f(a, n_rows, N, nl_dst, nh_dst, hoff):
    """dwt_zero_padding_f_stride_s on rows 0 .. n_rows-1 (src/libdwt.c:12118)."""
    if nl_dst or nh_dst:
        a[:n_rows, (N + 1) // 2:nl_dst] = 0
        a[:n_rows, hoff + N // 2:hoff + nh_dst] = 0


# ---- 2-D drivers --------------------------------------------------------------------------------------------
def fwd2d(a, size_i=None, j_max=-1, decompose_one=0, zero_padding=0):
    """dwt_interp53_2f_s in place on the float32 image a (size_o = a.shape); returns the level count."""
    soy, sox = a.shape
    siy, six = size_i or (soy, sox)
    j_limit = ceil_log2(max(sox, soy) if decompose_one else min(sox, soy))
    if j_max < 0 or j_max > j_limit:
        j_max = j_limit
    for j in range(j_max):
        osx, osy = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j)
        odx, ody = ceil_div_pow2(sox, j + 1), ceil_div_pow2(soy, j + 1)
        isx, isy = ceil_div_pow2(six, j), ceil_div_pow2(siy, j)
        _fwd_rows(a, osy, isx, odx)
        at = a.T
        _fwd_rows(at, osx, isy, ody)
        if zero_padding:
            _zero_f(a, osy, isx, odx, osx - odx, odx)
            _zero_f(at, osx, isy, ody, osy - ody, ody)
    return j_max


def inv2d(a, size_i=None, j_max=-1, decompose_one=0, zero_padding=0):
    """dwt_interp53_2i_s in place on the float32 image a."""
    soy, sox = a.shape
    siy, six = size_i or (soy, sox)
    j = ceil_log2(max(sox, soy) if decompose_one else min(sox, soy))
    if 0 <= j_max < j:
        j = j_max
    while j > 0:
        osx, osy = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j)
        odx, ody = ceil_div_pow2(sox, j - 1), ceil_div_pow2(soy, j - 1)
        idx_, idy = ceil_div_pow2(six, j - 1), ceil_div_pow2(siy, j - 1)
        _inv_rows(a, ody, idx_, osx)
        at = a.T
        _inv_rows(at, odx, idy, osy)
        if zero_padding:
            a[:ody, idx_:odx] = 0
            at[:odx, idy:ody] = 0
        j -= 1


# ---- 1-D drivers (on each row of a 2-D array: the lines of a batch) ------------------------------------------
def fwd1d(a, size_i=None, j_max=-1, zero_padding=0):
    """dwt_interp53_1f_s on every row of the float32 array a (n_lines x size_o); returns the level count."""
    so = a.shape[1]
    si = so if size_i is None else size_i
    j_limit = ceil_log2(so)
    if j_max < 0 or j_max > j_limit:
        j_max = j_limit
    n = a.shape[0]
    for j in range(j_max):
        os_, od, is_ = ceil_div_pow2(so, j), ceil_div_pow2(so, j + 1), ceil_div_pow2(si, j)
        if os_ > 1:  # lines_x = size_o_src_x
            _fwd_rows(a, n, is_, od)
        if zero_padding:
            _zero_f(a, n, is_, od, os_ - od, od)
    return j_max


def inv1d(a, size_i=None, j_max=-1, zero_padding=0):
    """dwt_interp53_1i_s on every row of a."""
    so = a.shape[1]
    si = so if size_i is None else size_i
    j = ceil_log2(so)
    if 0 <= j_max < j:
        j = j_max
    n = a.shape[0]
    while j > 0:
        os_, od, id_ = ceil_div_pow2(so, j), ceil_div_pow2(so, j - 1), ceil_div_pow2(si, j - 1)
        if od > 1:  # lines_x = size_o_dst_x
            _inv_rows(a, n, id_, os_)
        if zero_padding:
            a[:, id_:od] = 0
        j -= 1


class RefInterp53:
    """dwt_interp53_2f_s / _2i_s / _1f_s / _1i_s of the compiled reference."""

    def __init__(self):
        self.lib = C.CDLL(REF_SO)
        P, I = C.c_void_p, C.c_int
        self.lib.dwt_interp53_2f_s.argtypes = [P, I, I, I, I, I, I, C.POINTER(I), I, I]
        self.lib.dwt_interp53_2i_s.argtypes = [P, I, I, I, I, I, I, I, I, I]
        self.lib.dwt_interp53_1f_s.argtypes = [P, I, I, I, C.POINTER(I), I]
        self.lib.dwt_interp53_1i_s.argtypes = [P, I, I, I, I, I]
        for n in ("dwt_interp53_2f_s", "dwt_interp53_2i_s", "dwt_interp53_1f_s", "dwt_interp53_1i_s"):
            getattr(self.lib, n).restype = None

    def fwd2d(self, a, size_i=None, j_max=-1, decompose_one=0, zero_padding=0):
        soy, sox = a.shape
        siy, six = size_i or (soy, sox)
        j = C.c_int(j_max)
        self.lib.dwt_interp53_2f_s(a.ctypes.data, a.strides[0], 4, sox, soy, six, siy, C.byref(j), decompose_one, zero_padding)
        return j.value

    def inv2d(self, a, size_i=None, j_max=-1, decompose_one=0, zero_padding=0):
        soy, sox = a.shape
        siy, six = size_i or (soy, sox)
        self.lib.dwt_interp53_2i_s(a.ctypes.data, a.strides[0], 4, sox, soy, six, siy, j_max, decompose_one, zero_padding)

    def fwd1d(self, a, size_i=None, j_max=-1, zero_padding=0):
        so = a.shape[1]
        si = so if size_i is None else size_i
        jr = j_max
        for r in range(a.shape[0]):
            j = C.c_int(j_max)
            self.lib.dwt_interp53_1f_s(a[r].ctypes.data, 4, so, si, C.byref(j), zero_padding)
            jr = j.value
        return jr

    def inv1d(self, a, size_i=None, j_max=-1, zero_padding=0):
        so = a.shape[1]
        si = so if size_i is None else size_i
        for r in range(a.shape[0]):
            self.lib.dwt_interp53_1i_s(a[r].ctypes.data, 4, so, si, j_max, zero_padding)
