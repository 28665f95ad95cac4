"""Model of the stationary wavelet transform under a chosen border rule and of its inverse, in the style
of tests/swt_model.py.  With u = 1 << level, a filter g of 2c+1 taps and a plane x of N samples, for every p:

    conv_B(x, g, u)[p]:  y = +0.0f;  for k = -c .. +c:  y = fl32(y + fl32(x[B(p - u*k, N)] * g[k + c]))

B is the border map: `clip` (REPLICATE, the reference's rule) or `reflect` (SYMMETRIC, whole-sample symmetric extension):
reflect(i, 1) = 0, otherwise P = 2(N-1), m = i mod P taken non-negative, m > N-1 ? P - m : m.

Forward: swt_model / swt2d_model with B for clip.  Synthesis filters: the analysis taps with alternating signs around the
centre, sl[i] = (-1)^(i-CH) * gh[i] (low-pass, 2 CH + 1 taps) and sh[i] = (-1)^(i-CL) * gl[i] (high-pass).  Inverse, one 1-D
level: x = fl32(0.5f * fl32(conv_reflect(L, sl, u) + conv_reflect(H, sh, u))), levels from levels-1 down to 0.  One 2-D
level, columns first and then rows:

    Lr = 0.5f*(conv_y(LL, sl) + conv_y(LH, sh))   Hr = 0.5f*(conv_y(HL, sl) + conv_y(HH, sh))   A = 0.5f*(conv_x(Lr, sl) + conv_x(Hr, sh))

Operators on load: a detail plane passes through shape_model.apply_op (KEEP, ZERO, SCALE, HARD, SOFT) before it is
filtered.  `dtype=np.float64` restates everything in double (the filters stay the float32 values): what the filter
literals alone cost a round trip."""
import numpy as np

import shape_model as shp
import swt_model as sm

F32 = np.float32
REPLICATE, SYMMETRIC = 0, 1
KEEP, ZERO, SCALE, HARD, SOFT, COMPRESS = shp.KEEP, shp.ZERO, shp.SCALE, shp.HARD, shp.SOFT, shp.COMPRESS


def reflect(i, n):
    """whole-sample symmetric extension of the indices i into 0 .. n-1"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    P = 2 * (n - 1)
    m = np.mod(i, P)  # (non-negative)
    return np.where(m > n - 1, P - m, m)


def border_map(i, n, border):
    return reflect(i, n) if border == SYMMETRIC else np.clip(i, 0, n - 1)


def convolve(x, g, u, border, dtype=F32):
    """One dilated filter along the last axis under the border rule."""
    x = np.asarray(x, dtype=dtype)
    n = x.shape[-1]
    c = len(g) // 2
    p = np.arange(n, dtype=np.int64)
    y = np.zeros(x.shape, dtype=dtype)
    with np.errstate(all="ignore"):
        for k in range(-c, c + 1):
            idx = border_map(p - u * k, n, border)
            y = (y + (x[..., idx] * dtype(g[k + c])).astype(dtype)).astype(dtype)
    return y


def conv_y(x, g, u, border, dtype=F32):
    """convolve down the columns (axis -2)"""
    return np.swapaxes(convolve(np.swapaxes(x, -1, -2), g, u, border, dtype), -1, -2)


def synthesis(wavelet):
    """(sl, sh): the low-pass and the high-pass synthesis filter"""
    gl, gh = sm.FILTERS[wavelet]
    cl, ch = len(gl) // 2, len(gh) // 2
    sl = np.array([-v if (i - ch) % 2 else v for i, v in enumerate(gh)], F32)
    sh = np.array([-v if (i - cl) % 2 else v for i, v in enumerate(gl)], F32)
    return sl, sh


# ---- forward ---------------------------------------------------------------------------------------------------------------
def swt_levels(x, wavelet, levels, border=SYMMETRIC, dtype=F32):
    """(L planes, H planes), each (levels,) + x.shape; level l+1 reads L plane l"""
    gl, gh = sm.FILTERS[wavelet]
    x = np.asarray(x, dtype=dtype)
    L = np.zeros((levels,) + x.shape, dtype=dtype)
    H = np.zeros((levels,) + x.shape, dtype=dtype)
    cur = x
    for l in range(levels):
        L[l], H[l] = convolve(cur, gl, 1 << l, border, dtype), convolve(cur, gh, 1 << l, border, dtype)
        cur = L[l]
    return L, H


def swt2d_level(x, wavelet, level, border=SYMMETRIC, dtype=F32):
    """(LL, HL, LH, HH): rows, then columns"""
    gl, gh = sm.FILTERS[wavelet]
    u = 1 << level
    x = np.asarray(x, dtype=dtype)
    lr, hr = convolve(x, gl, u, border, dtype), convolve(x, gh, u, border, dtype)
    return conv_y(lr, gl, u, border, dtype), conv_y(hr, gl, u, border, dtype), conv_y(lr, gh, u, border, dtype), conv_y(hr, gh, u, border, dtype)


def swt2d_levels(x, wavelet, levels, border=SYMMETRIC, dtype=F32):
    """(LL planes (levels,) + x.shape, detail planes (levels, 3) + x.shape in the order HL, LH, HH)"""
    x = np.asarray(x, dtype=dtype)
    LL = np.zeros((levels,) + x.shape, dtype=dtype)
    D = np.zeros((levels, 3) + x.shape, dtype=dtype)
    cur = x
    for l in range(levels):
        LL[l], D[l, 0], D[l, 1], D[l, 2] = swt2d_level(cur, wavelet, l, border, dtype)
        cur = LL[l]
    return LL, D


# ---- inverse ---------------------------------------------------------------------------------------------------------------
def on_load(plane, op, param, dtype=F32):
    """the plane as the inverse reads it under operator `op`"""
    if op == COMPRESS:
        raise ValueError("COMPRESS is not an operator on load")
    return plane if op == KEEP else shp.apply_op(plane, op, param).astype(dtype)


def _half_sum(a, b, dtype):
    with np.errstate(all="ignore"):
        return (dtype(0.5) * (a + b).astype(dtype)).astype(dtype)


def iswt_level(L, H, wavelet, level, dtype=F32):
    sl, sh = synthesis(wavelet)
    u = 1 << level
    return _half_sum(convolve(L, sl, u, SYMMETRIC, dtype), convolve(H, sh, u, SYMMETRIC, dtype), dtype)


def iswt_levels(L_last, H, wavelet, ops=None, params=None, dtype=F32):
    """the rows from the last level's L plane and the H planes (levels,) + L_last.shape; ops / params: one per level"""
    cur = np.asarray(L_last, dtype=dtype)
    for l in range(len(H) - 1, -1, -1):
        h = H[l] if ops is None else on_load(H[l], ops[l], params[l], dtype)
        cur = iswt_level(cur, h, wavelet, l, dtype)
    return cur


def iswt2d_level(LL, HL, LH, HH, wavelet, level, dtype=F32):
    sl, sh = synthesis(wavelet)
    u = 1 << level
    lr = _half_sum(conv_y(LL, sl, u, SYMMETRIC, dtype), conv_y(LH, sh, u, SYMMETRIC, dtype), dtype)
    hr = _half_sum(conv_y(HL, sl, u, SYMMETRIC, dtype), conv_y(HH, sh, u, SYMMETRIC, dtype), dtype)
    return _half_sum(convolve(lr, sl, u, SYMMETRIC, dtype), convolve(hr, sh, u, SYMMETRIC, dtype), dtype)


def iswt2d_levels(LL_last, D, wavelet, ops=None, params=None, dtype=F32):
    """the images from the last level's LL and the detail planes (levels, 3) + LL_last.shape; ops / params: 3 * levels
    entries, the plane's at index 3*l + k-1 (HL, LH, HH)"""
    cur = np.asarray(LL_last, dtype=dtype)
    for l in range(len(D) - 1, -1, -1):
        d = [D[l, k] if ops is None else on_load(D[l, k], ops[3 * l + k], params[3 * l + k], dtype) for k in range(3)]
        cur = iswt2d_level(cur, d[0], d[1], d[2], wavelet, l, dtype)
    return cur


def interior(n, levels, wavelet):
    """the samples p of a line of n that no border rule reaches within `levels` levels: CL*(2^J - 1) <= p < n - CL*(2^J - 1)"""
    reach = (len(sm.FILTERS[wavelet][0]) // 2) * ((1 << levels) - 1)
    return slice(reach, max(n - reach, reach))
