"""Model of the 2-D stationary wavelet transform: libdwt's two row functions (swt_cdf97_f_ex_stride_s /
swt_cdf53_f_ex_stride_s, src/swt.c; tests/swt_model.py) applied separably.  With u = 1 << l and A the level's input (the
image at level 0, LL of level l-1 after that):

    Lr = conv_x(A, g_low)    Hr = conv_x(A, g_high)                                     (along x, for every row)
    LL = conv_y(Lr, g_low)   LH = conv_y(Lr, g_high)   HL = conv_y(Hr, g_low)   HH = conv_y(Hr, g_high)   (along y)

every conv swt_model.convolve: float32, product and sum rounded separately, from +0.0f, borders replicated.  No direction
is skipped: a 1-row image takes its column pass with N = 1.  Band names as enum dwt_subbands: HL is high-pass along a row.

* `swt2d_level`, `swt2d_levels` -- the numpy float32 restatement;
* `make_input` -- seeded images: normal, small integers, all-subnormal (`tiny`), and the whole float range with its
  non-finite and overflowing samples confined to the top-left 4 x 4 corner (elsewhere they would spread through most of
  the coefficients within a few levels and hide everything);
* `CASES` -- what tests/golden/swt2d.npz holds: the reference's two functions run over the rows (stride 4) and then over
  the columns (stride = pitch), written by scripts/gen_swt2d_golden.py."""
import os

import numpy as np

import swt_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "swt2d.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "swt2d_manifest.json")

F32 = np.float32
TINY = np.finfo(F32).tiny  # FLT_MIN
BANDS = ("HL", "LH", "HH")  # detail band k = 1, 2, 3 at index k-1


def conv_y(x, g, u):
    """swt_model.convolve down the columns (axis -2)"""
    return np.swapaxes(sm.convolve(np.swapaxes(x, -1, -2), g, u), -1, -2)


def swt2d_level(x, wavelet, level):
    """(LL, HL, LH, HH) of one level at dilation 1 << level of an image (or of every image of a stack)."""
    gl, gh = sm.FILTERS[wavelet]
    u = 1 << level
    x = np.asarray(x, dtype=F32)
    lr, hr = sm.convolve(x, gl, u), sm.convolve(x, gh, u)
    return conv_y(lr, gl, u), conv_y(hr, gl, u), conv_y(lr, gh, u), conv_y(hr, gh, u)


def swt2d_levels(x, wavelet, levels):
    """(LL planes of shape (levels,) + x.shape, detail planes of shape (levels, 3) + x.shape in the order HL, LH, HH);
    level l+1 reads LL plane l."""
    x = np.asarray(x, dtype=F32)
    LL = np.zeros((levels,) + x.shape, dtype=F32)
    D = np.zeros((levels, 3) + x.shape, dtype=F32)
    cur = x
    for l in range(levels):
        LL[l], D[l, 0], D[l, 1], D[l, 2] = swt2d_level(cur, wavelet, l)
        cur = LL[l]
    return LL, D


KINDS = ("normal", "small_ints", "tiny", "float_range")
CORNER = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (3, 3))  # where the special values of float_range go


def make_input(seed, kind, size_y, size_x):
    """one seeded image of size_y rows and size_x columns"""
    if kind in ("normal", "small_ints"):
        return sm.make_input(seed, kind, size_y, size_x)
    if kind == "tiny":  # every sample subnormal or zero
        rng = np.random.default_rng(seed)
        a = (rng.standard_normal((size_y, size_x)) * (TINY / 4)).astype(F32)
        r = rng.random((size_y, size_x))
        a[r < 0.06] = F32(0.0)
        a[(r >= 0.06) & (r < 0.12)] = F32(-0.0)
        return a
    assert kind == "float_range"
    a = sm.make_input(seed, kind, size_y, size_x)
    with np.errstate(invalid="ignore"):
        wild = ~np.isfinite(a) | (np.abs(a) > F32(1e38))
    wild[:4, :4] = False
    a[wild] = F32(0.0)
    special = (F32(np.nan), F32(np.inf), F32(-np.inf), F32(3e38), F32(-3e38), F32(TINY / 8))
    for (y, x), v in zip(CORNER, special):
        if y < size_y and x < size_x:
            a[y, x] = v
    return a


def nonfinite_share(*arrays):
    """the share of non-finite values over all the arrays"""
    n = sum(a.size for a in arrays)
    return sum(int((~np.isfinite(a)).sum()) for a in arrays) / max(n, 1)


def subnormal_share(*arrays):
    """the share of subnormal values (non-zero, magnitude below FLT_MIN) over all the arrays"""
    n = sum(a.size for a in arrays)
    with np.errstate(invalid="ignore"):
        return sum(int(((a != 0) & (np.abs(a) < TINY)).sum()) for a in arrays) / max(n, 1)


NONFINITE_CAP = 0.10   # float_range: at most this share of the expected coefficients may be non-finite
SUBNORMAL_FLOOR = 0.5  # tiny: at least this share of the expected coefficients must be subnormal


def check_kind(kind, LL, D):
    """the two conditions on what a case compares: the detail planes of every level and the last LL"""
    if kind == "float_range":
        share = nonfinite_share(D, LL[-1:])
        assert share <= NONFINITE_CAP, ("float_range: non-finite share", share)
    if kind == "tiny":
        share = subnormal_share(D, LL[-1:])
        assert share >= SUBNORMAL_FLOOR, ("tiny: subnormal share", share)


# (seed, wavelet, kind, size_y, size_x, levels): the detail planes of every level and the last LL are stored
CASES = [
    (4101, "cdf97_s", "normal", 1, 1, 3),
    (4102, "cdf53_s", "small_ints", 1, 9, 4),
    (4103, "cdf97_s", "normal", 7, 1, 3),
    (4104, "cdf53_s", "tiny", 2, 3, 5),
    (4105, "cdf97_s", "tiny", 37, 53, 7),
    (4106, "cdf53_s", "float_range", 40, 150, 3),
    (4107, "cdf97_s", "float_range", 96, 120, 2),
    (4108, "cdf97_s", "small_ints", 65, 30, 4),
    (4109, "cdf53_s", "normal", 30, 33, 6),
]
