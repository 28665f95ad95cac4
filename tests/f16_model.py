"""The float CDF 9/7 on IEEE binary16 storage (DWT_HIP_CDF97_H, dwt_cdf97_2f_h / dwt_cdf97_2i_h), restated
with the float oracle and numpy.

A multi-level call is the float transform's ONE-level step composed with a rounding per level:

  forward level j   the level's frame (outer size ceil(size_o / 2^j), inner size ceil(size_i / 2^j)) is converted
                    binary16 -> binary32 (exact), ONE level of dwt_cdf97_2f_s is applied to it, and the whole frame is
                    converted back, round to nearest even (astype(np.float16): overflow to +-Inf, subnormals kept);
  inverse level j   the same with ONE level of dwt_cdf97_2i_s on the frame of level j - 1, from the deepest level up.

The level count is clamped as the reference clamps it (ceil(log2(min side)), of the max side with decompose_one).  The
one-level calls pass decompose_one = 1: the flag enters the reference's level count only, and a one-level call on a frame
with a one-line direction would otherwise clamp itself to zero levels.  `rounded=False` leaves the rounding out -- the
chain of one-level calls in binary32, which must equal the oracle's multi-level transform bit for bit
(assert_chain_is_multilevel; tests/test_f16.py, scripts/gen_h16_golden.py)."""
import numpy as np

import oraclelib

_orc = None


def oracle():
    global _orc
    if _orc is None:
        _orc = oraclelib.Oracle()
    return _orc


def ceil_div_pow2(i, j):
    return (i + (1 << j) - 1) >> j


def ceil_log2(x):
    n = 0
    while (1 << n) < x:
        n += 1
    return n


def fwd_levels(size_o, j_max, decompose_one=0):
    """size_o = (x, y); the level count a forward call runs and reports."""
    lim = ceil_log2(max(size_o) if decompose_one else min(size_o))
    return lim if (j_max < 0 or j_max > lim) else j_max


def inv_levels(size_o, j_max, decompose_one=0):
    lim = ceil_log2(max(size_o) if decompose_one else min(size_o))
    return j_max if 0 <= j_max < lim else lim


def _sizes(a, size_o, size_i):
    h, w = a.shape
    so = size_o if size_o else (w, h)
    si = size_i if size_i else so
    assert so[0] <= w and so[1] <= h
    return so, si


def _level(lib, name, a, j, so, si, zero_padding, rounded):
    wo, ho = ceil_div_pow2(so[0], j), ceil_div_pow2(so[1], j)
    wi, hi = ceil_div_pow2(si[0], j), ceil_div_pow2(si[1], j)
    box = np.ascontiguousarray(a[:ho, :wo], np.float32)
    if "2f" in name:
        assert lib.fwd(name, box, 1, size_o=(wo, ho), size_i=(wi, hi), decompose_one=1, zero_padding=zero_padding) == 1
    else:
        lib.inv(name, box, 1, size_o=(wo, ho), size_i=(wi, hi), decompose_one=1, zero_padding=zero_padding)
    with np.errstate(over="ignore", invalid="ignore"):
        a[:ho, :wo] = box.astype(np.float16) if rounded else box


def fwd2d(a, size_o=None, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, rounded=True, lib=None):
    """In place on the 2-D array `a` (rows = y): np.float16, or np.float32 with rounded=False.  size_o / size_i are (x, y)
    pairs and default to the array's shape.  Returns the level count."""
    assert a.dtype == (np.float16 if rounded else np.float32) and a.ndim == 2
    lib = lib or oracle()
    so, si = _sizes(a, size_o, size_i)
    J = fwd_levels(so, j_max, decompose_one)
    for j in range(J):
        _level(lib, "cdf97_2f_s", a, j, so, si, zero_padding, rounded)
    return J


def inv2d(a, size_o=None, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, rounded=True, lib=None):
    assert a.dtype == (np.float16 if rounded else np.float32) and a.ndim == 2
    lib = lib or oracle()
    so, si = _sizes(a, size_o, size_i)
    J = inv_levels(so, j_max, decompose_one)
    for j in range(J, 0, -1):
        _level(lib, "cdf97_2i_s", a, j - 1, so, si, zero_padding, rounded)
    return J


def same_bits(a, b):
    """binary32 arrays: identical bits where neither is NaN, NaNs at identical positions."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def assert_chain_is_multilevel(x, size_o=None, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, lib=None):
    """The model without its rounding equals the multi-level float transform bit for bit, forward and inverse: the
    per-level composition (frames, clamps, decompose_one, one-line directions) is the float transform's own."""
    lib = lib or oracle()
    x = np.ascontiguousarray(x, np.float32)
    so, si = _sizes(x, size_o, size_i)
    chain, whole = x.copy(), x.copy()
    J = fwd2d(chain, so, si, j_max, decompose_one, zero_padding, rounded=False, lib=lib)
    jw = lib.fwd("cdf97_2f_s", whole, j_max, size_o=so, size_i=si, decompose_one=decompose_one, zero_padding=zero_padding)
    assert J == jw and same_bits(chain, whole), ("forward chain != multi-level transform", x.shape, so, si, j_max, decompose_one, zero_padding)
    inv2d(chain, so, si, J, decompose_one, zero_padding, rounded=False, lib=lib)
    lib.inv("cdf97_2i_s", whole, J, size_o=so, size_i=si, decompose_one=decompose_one, zero_padding=zero_padding)
    assert same_bits(chain, whole), ("inverse chain != multi-level transform", x.shape, so, si, j_max, decompose_one, zero_padding)
    return J
