"""A numpy restatement of the reversible int16 CDF 5/3 transform in JPEG 2000 order (DWT_HIP_CDF53_I16,
dwt_cdf53_2f_i16 / dwt_cdf53_2i_i16).  The arithmetic is normative:

  - a forward level lifts every column first, then every row (ITU-T T.800 F.3.2, 2D_SD); the inverse level every row
    first, then every column -- the exact mirror;
  - forward, odd sample:  d -= (l + r) >> 1;  forward, even sample:  s += (dl + dr + 2) >> 2;  the inverse the same terms
    with the opposite sign in the opposite order (F.3.8.1);
  - every sum and shift is evaluated in `int` on sign-extended operands and the result is truncated to 16 bits when it is
    stored (the element step cdf53_vert_2x1_i16 of the reference's core, examples/cores/cores.c, as C evaluates it);
  - line ends by whole-sample symmetric reflection; a line of one sample is left as it is.

Consequence: the inverse restores every int16 image bit for bit, wrapped values included.  The layout is multi-level
Mallat with the geometry and j_max rules of dwt_cdf53_2f_i.

`rows_first=True` gives the variant that lifts rows before columns (and undoes columns before rows), the order of the
int32 dwt_cdf53_2f_i: tests tie the lifting formulas to the existing oracle through it."""
import numpy as np


def ceil_log2(x):
    j = 0
    while (1 << j) < x:
        j += 1
    return j


def ceil_div_pow2(x, j):
    return (x + (1 << j) - 1) >> j


def _narrow(t):
    """int32 values truncated to 16 bits, sign-extended again (what a store to int16_t and the next load give)."""
    return t.astype(np.int16).astype(np.int32)


def fwd_lines(t):
    """The forward lifting of the lines t (n_lines x N, any int type holding int16 values) -> interleaved, int32."""
    t = np.array(t, dtype=np.int32, copy=True)
    N = t.shape[1]
    if N < 2:
        return t
    ev = t[:, 0::2]
    # the right neighbour of the last odd sample of an even-length line is the reflected even sample N - 2
    r = np.concatenate([ev[:, 1:], ev[:, -1:]], axis=1) if N % 2 == 0 else ev[:, 1:]
    d = _narrow(t[:, 1::2] - ((ev[:, :r.shape[1]] + r) >> 1))
    # the left neighbour of sample 0 is d[0] (reflection); the right neighbour of the last even sample of an odd-length
    # line is the reflected d[-1]
    dl = np.concatenate([d[:, :1], d], axis=1)
    dr = np.concatenate([d, d[:, -1:]], axis=1)
    n_ev = ev.shape[1]
    s = _narrow(ev + ((dl[:, :n_ev] + dr[:, :n_ev] + 2) >> 2))
    t[:, 0::2] = s
    t[:, 1::2] = d
    return t


def inv_lines(t):
    """The inverse of fwd_lines on interleaved lines (n_lines x N)."""
    t = np.array(t, dtype=np.int32, copy=True)
    N = t.shape[1]
    if N < 2:
        return t
    d = t[:, 1::2]
    dl = np.concatenate([d[:, :1], d], axis=1)
    dr = np.concatenate([d, d[:, -1:]], axis=1)
    n_ev = (N + 1) // 2
    ev = _narrow(t[:, 0::2] - ((dl[:, :n_ev] + dr[:, :n_ev] + 2) >> 2))
    r = np.concatenate([ev[:, 1:], ev[:, -1:]], axis=1) if N % 2 == 0 else ev[:, 1:]
    od = _narrow(d + ((ev[:, :r.shape[1]] + r) >> 1))
    t[:, 0::2] = ev
    t[:, 1::2] = od
    return t


def _fwd_rows(a, n_rows, N, hoff):
    """rows 0 .. n_rows-1 of a: samples [0, N) -> L at [0, ceil(N/2)), H at hoff (a line of one sample stays)."""
    if N < 2 or n_rows == 0:
        return
    t = fwd_lines(a[:n_rows, :N])
    a[:n_rows, :(N + 1) // 2] = t[:, 0::2].astype(np.int16)
    a[:n_rows, hoff:hoff + N // 2] = t[:, 1::2].astype(np.int16)


def _inv_rows(a, n_rows, N, hoff):
    if N < 2 or n_rows == 0:
        return
    t = np.empty((n_rows, N), np.int32)
    t[:, 0::2] = a[:n_rows, :(N + 1) // 2]
    t[:, 1::2] = a[:n_rows, hoff:hoff + N // 2]
    a[:n_rows, :N] = inv_lines(t).astype(np.int16)


def _zero_f(a, n_rows, N, nl_dst, nh_dst, hoff):
    if nl_dst or nh_dst:
        a[:n_rows, (N + 1) // 2:nl_dst] = 0
        a[:n_rows, hoff + N // 2:hoff + nh_dst] = 0


def fwd2d(a, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, rows_first=False):
    """dwt_cdf53_2f_i16 in place on the int16 image a (size_o = a.shape); returns the level count."""
    assert a.dtype == np.int16
    soy, sox = a.shape
    siy, six = size_i or (soy, sox)
    j_limit = ceil_log2(max(sox, soy) if decompose_one else min(sox, soy))
    if j_max < 0 or j_max > j_limit:
        j_max = j_limit
    at = a.T
    for j in range(j_max):
        osx, osy = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j)
        odx, ody = ceil_div_pow2(sox, j + 1), ceil_div_pow2(soy, j + 1)
        isx, isy = ceil_div_pow2(six, j), ceil_div_pow2(siy, j)
        if rows_first:
            _fwd_rows(a, osy, isx, odx)
            _fwd_rows(at, osx, isy, ody)
        else:
            _fwd_rows(at, osx, isy, ody)  # every column ...
            _fwd_rows(a, osy, isx, odx)   # ... then every row
        if zero_padding:
            _zero_f(a, osy, isx, odx, osx - odx, odx)
            _zero_f(at, osx, isy, ody, osy - ody, ody)
    return j_max


def inv2d(a, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, rows_first=False):
    """dwt_cdf53_2i_i16 in place on the int16 image a.  rows_first names the FORWARD order that is undone."""
    assert a.dtype == np.int16
    soy, sox = a.shape
    siy, six = size_i or (soy, sox)
    j = ceil_log2(max(sox, soy) if decompose_one else min(sox, soy))
    if 0 <= j_max < j:
        j = j_max
    at = a.T
    while j > 0:
        osx, osy = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j)
        odx, ody = ceil_div_pow2(sox, j - 1), ceil_div_pow2(soy, j - 1)
        idx_, idy = ceil_div_pow2(six, j - 1), ceil_div_pow2(siy, j - 1)
        if rows_first:
            _inv_rows(at, odx, idy, osy)
            _inv_rows(a, ody, idx_, osx)
        else:
            _inv_rows(a, ody, idx_, osx)  # every row ...
            _inv_rows(at, odx, idy, osy)  # ... then every column
        if zero_padding:
            a[:ody, idx_:odx] = 0
            at[:odx, idy:ody] = 0
        j -= 1


# ---- the single-level INTERLEAVED form the reference's core produces (scripts/gen_i16_golden.py) --------------------
def core_fwd(img):
    """One forward level, columns then rows, the result left interleaved in place (what cores2f_cdf53_v2x2_i16 writes)."""
    a = np.array(img, dtype=np.int16, copy=True)
    if a.shape[0] >= 2:
        a[:] = fwd_lines(a.T).T.astype(np.int16)
    if a.shape[1] >= 2:
        a[:] = fwd_lines(a).astype(np.int16)
    return a


def core_inv(img):
    """The inverse of core_fwd: rows, then columns."""
    a = np.array(img, dtype=np.int16, copy=True)
    if a.shape[1] >= 2:
        a[:] = inv_lines(a).astype(np.int16)
    if a.shape[0] >= 2:
        a[:] = inv_lines(a.T).T.astype(np.int16)
    return a


def mallat_of(il):
    """The Mallat arrangement of one interleaved level: [LL HL; LH HH]."""
    return np.block([[il[0::2, 0::2], il[0::2, 1::2]], [il[1::2, 0::2], il[1::2, 1::2]]])
