"""Model of libdwt's stationary wavelet transform (swt_cdf97_f_ex_stride_s / swt_cdf53_f_ex_stride_s, src/swt.c, over
dwt_util_convolve1_s, src/util.c:5-48, and the saturating accessors of src/signal.c:43-93), written from the reference's
definition.  With u = 1 << level, a filter g of 2c+1 taps and the level's input x of N samples, for every p:

    y = 0.0f;  for k = -c .. +c:  y = fl32(y + fl32(x[clamp(p - u*k, 0, N-1)] * g[k + c]));  out[p] = y

float32, product and sum rounded separately, from +0.0f, the taps in that order, borders replicated.  Both filters read
the same input; level l+1 filters the low-pass plane of level l.

* `swt_level`, `swt_levels` -- the numpy float32 restatement;
* `make_input` -- seeded rows: normal, small integers (ties, both zeros), the whole float range (subnormals, +-0, +-Inf,
  NaN, values near overflow);
* `CASES` -- what tests/golden/swt.npz holds: the outputs of the reference's two functions, written by
  scripts/gen_swt_golden.py."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "swt.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "swt_manifest.json")

F32 = np.float32
MAX_LEVELS = 24

# the filters as the reference spells them in decimal (literals of type double), rounded to float32
FILTERS = {
    "cdf97_s": (np.array([+0.03782846, -0.02384947, -0.11062438, +0.37740287, +0.85269880, +0.37740287, -0.11062438, -0.02384947,
                          +0.03782846], dtype=np.float64).astype(F32),
                np.array([+0.06453887, -0.04068942, -0.41809219, +0.78848559, -0.41809219, -0.04068942, +0.06453887],
                         dtype=np.float64).astype(F32)),
    "cdf53_s": (np.array([-0.17677669, +0.35355338, +1.06066012, +0.35355338, -0.17677669], dtype=np.float64).astype(F32),
                np.array([-0.35355338, +0.70710677, -0.35355338], dtype=np.float64).astype(F32)),
}
WAVELETS = tuple(FILTERS)


def convolve(x, g, u):
    """One dilated filter over a row (or over every row of a 2-D array, along the last axis)."""
    x = np.asarray(x, dtype=F32)
    n = x.shape[-1]
    c = len(g) // 2
    p = np.arange(n, dtype=np.int64)
    y = np.zeros(x.shape, dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(-c, c + 1):
            idx = np.clip(p - u * k, 0, n - 1)
            y = (y + (x[..., idx] * g[k + c]).astype(F32)).astype(F32)
    return y


def swt_level(x, wavelet, level):
    """(L, H) of one level at dilation 1 << level."""
    gl, gh = FILTERS[wavelet]
    return convolve(x, gl, 1 << level), convolve(x, gh, 1 << level)


def swt_levels(x, wavelet, levels):
    """(L planes, H planes), each of shape (levels,) + x.shape: plane l is level l's output, level l+1 reads L plane l."""
    x = np.asarray(x, dtype=F32)
    L = np.zeros((levels,) + x.shape, dtype=F32)
    H = np.zeros((levels,) + x.shape, dtype=F32)
    cur = x
    for l in range(levels):
        L[l], H[l] = swt_level(cur, wavelet, l)
        cur = L[l]
    return L, H


KINDS = ("normal", "small_ints", "float_range")


def make_input(seed, kind, n_lines, n):
    """n_lines seeded rows of n samples."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((n_lines, n)).astype(F32)
    if kind == "small_ints":  # ties and both zeros
        a = rng.integers(-3, 4, (n_lines, n)).astype(F32)
        a[rng.random((n_lines, n)) < 0.1] = F32(-0.0)
        return a
    assert kind == "float_range"
    a = rng.standard_normal((n_lines, n)).astype(F32)
    r = rng.random((n_lines, n))
    tiny = np.finfo(F32).tiny
    a[r < 0.30] *= F32(tiny / 4)  # subnormals and the smallest normals
    a[(r >= 0.30) & (r < 0.36)] = F32(0.0)
    a[(r >= 0.36) & (r < 0.42)] = F32(-0.0)
    big = (r >= 0.42) & (r < 0.52)
    a[big] = (np.sign(a[big]) * F32(1e30) * (F32(1) + np.abs(a[big]))).astype(F32)  # near 1e30: sums stay finite
    near = (r >= 0.52) & (r < 0.53)
    a[near] = np.where(a[near] < 0, F32(-3e38), F32(3e38))  # products and sums overflow
    a[(r >= 0.530) & (r < 0.533)] = F32(np.inf)
    a[(r >= 0.533) & (r < 0.536)] = F32(-np.inf)
    a[(r >= 0.536) & (r < 0.539)] = F32(np.nan)
    if n >= 7:  # every special value at least once, in the last row
        a[-1, [0, n // 3, n // 2, n - 2, n - 1]] = [F32(np.nan), F32(np.inf), F32(3e38), F32(-np.inf), F32(tiny / 8)]
    return a


def same(a, b):
    """bit-equal float32 arrays, NaNs of any payload equal"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# (seed, wavelet, kind, n, levels): one row each, the reference's two functions chained level by level
CASES = [
    (3101, "cdf97_s", "normal", 1, 3),
    (3102, "cdf53_s", "normal", 2, 3),
    (3103, "cdf97_s", "small_ints", 3, 4),
    (3104, "cdf53_s", "float_range", 7, 5),
    (3105, "cdf97_s", "float_range", 100, 10),
    (3106, "cdf53_s", "small_ints", 257, 10),
    (3107, "cdf97_s", "normal", 257, 14),
    (3108, "cdf53_s", "float_range", 1000, 6),
    (3109, "cdf97_s", "normal", 4096, 4),
    (3110, "cdf53_s", "normal", 4096, 3),
    (3111, "cdf97_s", "float_range", 64, 11),
    (3112, "cdf53_s", "small_ints", 77, 3),
]
