"""Numpy model of the per-band coefficient operators, the log / exp maps and the universal threshold,
written from their definition:

* `levels`, `slots` -- the level count of a call and the slot geometry (the bands of dwt_util_subband_s: slot 3(j-1) +
  {0, 1, 2} is HL, LH, HH of level j, slot 3J is LL of level J);
* `apply_op` / `apply_table` -- the operators in float32 arithmetic as the contract writes them; COMPRESS, LOG and EXP
  evaluate in float64 and round to float32 once (`how="f64"`) or call the host libm's powf / logf / expf through ctypes
  (`how="libm"`: what the reference's programs produce);
* `threshold` -- the universal threshold from the median magnitude of the Mallat HH(1) band, finished in float32;
* `ulps` -- the distance of two float32 arrays in units of the last place;
* `CASES`, `make_input`, `make_table` -- the seeded cases tests/golden/shape.npz holds (scripts/gen_shape_golden.py).
"""
import ctypes as C
import ctypes.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shape.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "shape_manifest.json")
F32 = np.float32

KEEP, ZERO, SCALE, HARD, SOFT, COMPRESS = range(6)
OP_NAMES = ("keep", "zero", "scale", "hard", "soft", "compress")
LOG, EXP = "log", "exp"

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.argtypes = [C.c_float, C.c_float]
for _n in ("powf", "logf", "expf"):
    getattr(_libm, _n).restype = C.c_float
_libm.logf.argtypes = [C.c_float]
_libm.expf.argtypes = [C.c_float]


def _each(fn, x, *more):
    x = np.ascontiguousarray(x, F32)
    return np.array([fn(float(v), *more) for v in x.reshape(-1)], dtype=F32).reshape(x.shape)


def ceil_log2(x):
    n = 0
    while n < 31 and (1 << n) < x:
        n += 1
    return n


def cdiv_pow2(x, j):
    return (x + (1 << j) - 1) >> j


def levels(sox, soy, j_max=-1):
    """j_max < 0: the transforms' default for these sizes (the smaller side; a single row or column: its length);
    otherwise j_max, at most ceil(log2) of the larger side."""
    lo, hi = min(sox, soy), max(sox, soy)
    if j_max < 0:
        return ceil_log2(hi if lo <= 1 else lo)
    return min(j_max, ceil_log2(hi))


def slots(sox, soy, six, siy, J):
    """[(x0, y0, w, h)] of the 3J + 1 slots"""
    out = []
    for j in range(1, J + 1):
        hx, hy = cdiv_pow2(six, j - 1) // 2, cdiv_pow2(siy, j - 1) // 2
        lx, ly = cdiv_pow2(six, j), cdiv_pow2(siy, j)
        ox, oy = cdiv_pow2(sox, j), cdiv_pow2(soy, j)
        out += [(ox, 0, hx, ly), (0, oy, lx, hy), (ox, oy, hx, hy)]
    out.append((0, 0, cdiv_pow2(six, J), cdiv_pow2(siy, J)))
    return out


def apply_op(c, op, a, how="f64"):
    """one operator over a float32 array -> float32 array; NaN stays under everything but ZERO"""
    c = np.ascontiguousarray(c, F32)
    a = F32(a)
    nan = np.isnan(c)
    with np.errstate(all="ignore"):
        if op == KEEP:
            return c.copy()
        if op == ZERO:
            return np.zeros_like(c)
        if op == SCALE:
            r = (c * a).astype(F32)
        elif op == HARD:
            r = np.where(np.abs(c) > a, c, F32(0))
        elif op == SOFT:
            r = np.where(c > a, (c - a).astype(F32), np.where(c < -a, (c + a).astype(F32), F32(0)))
        elif op == COMPRESS:
            mag = np.abs(c)
            p = np.power(mag.astype(np.float64), np.float64(a)).astype(F32) if how == "f64" else _each(_libm.powf, mag, float(a))
            r = (np.where(c > 0, F32(1), F32(-1)) * p).astype(F32)
        elif op == LOG:
            s = (c + a).astype(F32)
            r = np.log(s.astype(np.float64)).astype(F32) if how == "f64" else _each(_libm.logf, s)
        elif op == EXP:
            e = np.exp(c.astype(np.float64)).astype(F32) if how == "f64" else _each(_libm.expf, c)
            r = (e - a).astype(F32)
        else:
            raise ValueError("unknown operator %r" % (op,))
    return np.where(nan, c, r).astype(F32)


def apply_table(img, sox, soy, six, siy, J, ops, params, how="f64"):
    """the table over a frame (rows of img; img may be wider / taller than the frame) -> a new array"""
    out = np.array(img, dtype=F32, copy=True)
    for (x0, y0, w, h), op, a in zip(slots(sox, soy, six, siy, J), ops, params):
        if op != KEEP and w and h:
            out[y0:y0 + h, x0:x0 + w] = apply_op(img[y0:y0 + h, x0:x0 + w], op, a, how)
    return out


def hh1(img, w, h):
    return img[h - h // 2:h, w - w // 2:w]


def abs_median(band):
    v = np.sort(np.abs(np.ascontiguousarray(band, F32)).reshape(-1), kind="stable")
    return F32(v[len(v) // 2])


def threshold_input(img, w, h):
    """a copy of img whose HH(1) band holds no NaN (the reference's comparator is no order there: the median is not pinned)"""
    out = np.array(img, dtype=F32, copy=True)
    band = hh1(out, w, h)
    band[np.isnan(band)] = 0
    return out


def threshold(img, w, h):
    """(med|HH(1)| / 0.6745f) * sqrtf(2.f * logf((float)(w * h))), every step float32"""
    sigma = F32(abs_median(hh1(img, w, h)) / F32(0.6745))
    spread = np.sqrt(F32(F32(2) * F32(_libm.logf(float(F32(w * h))))), dtype=F32)
    return F32(sigma * spread)


def ulps(a, b):
    """distance in float32 units of the last place (0 where the bits agree or both are NaN; huge where only one is NaN)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)

    d = np.abs(key(a) - key(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 1 << 40, d))


def same(got, want):
    """the same bits wherever neither side is a NaN, NaNs at the same places (payloads are not compared)"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


# ---- seeded cases ------------------------------------------------------------------------------------------------------
PARAM = {KEEP: 0.0, ZERO: 0.0, SCALE: -1.75, HARD: 0.5, SOFT: 0.5, COMPRESS: 0.7}
# name -> (sox, soy, six, siy, j_max, table kind); `fixture`: its results are part of tests/golden/shape.npz
CASES = {
    "odd": (37, 29, 37, 29, 3, "mixed"),
    "deep": (64, 64, 64, 64, 6, "mixed"),
    "tiny": (5, 3, 5, 3, -1, "mixed"),
    "row": (130, 1, 130, 1, -1, "mra"),
    "column": (1, 130, 1, 130, -1, "mra"),
    "inner": (96, 80, 90, 77, 3, "mixed"),
    "soft": (37, 29, 37, 29, 3, "soft"),
    "compress": (37, 29, 37, 29, 3, "compress"),
    "hdr": (64, 48, 64, 48, -1, "compress"),
}
BIG = (1024, 1024, 1024, 1024, 5, "mixed")  # the multi-chunk mapping: checked against the model alone


def make_input(seed, h, w):
    """normal samples with the values the operators branch on: both zeros, subnormals, both infinities, NaN, the
    thresholds themselves and their neighbours, magnitudes near overflow"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((h, w)) * 0.8).astype(F32)
    tiny = np.finfo(F32).tiny
    special = np.array([0.0, -0.0, tiny * 0.5, -tiny * 0.25, 1e-45, np.inf, -np.inf, np.nan, 0.5, -0.5,
                        np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(-0.5), F32(-1)), np.nextafter(F32(0.5), F32(0)),
                        3.0e38, -3.0e38, 2.5e38, 1.0, -1.0, tiny, -tiny], dtype=F32)
    pick = rng.random((h, w)) < 0.2
    a[pick] = rng.choice(special, size=int(pick.sum()))
    flat = a.reshape(-1)
    n = min(len(special), len(flat))
    flat[rng.permutation(len(flat))[:n]] = special[:n]  # each special at least once where there is room
    return a


def make_table(kind, n_slots, shift=0):
    """(ops, params) int32 / float32.  mixed: the operators in turn from slot to slot; mra: slot 3 + shift kept (H of
    level 2 of a row; shift 1: of a column), the rest zeroed; soft / compress: that operator on every detail slot, LL kept"""
    if kind == "mixed":
        ops = [(k + shift) % 6 for k in range(n_slots)]
    elif kind == "mra":
        ops = [ZERO] * n_slots
        ops[3 + shift] = KEEP
    else:
        ops = [SOFT if kind == "soft" else COMPRESS] * (n_slots - 1) + [KEEP]
    return np.array(ops, np.int32), np.array([PARAM[o] for o in ops], F32)


def case_seed(name):
    return 7000 + 31 * sorted(CASES).index(name)


def case_arrays(name):
    """(input, J, ops, params) of a fixture case"""
    sox, soy, six, siy, j_max, kind = CASES[name]
    J = levels(sox, soy, j_max)
    ops, params = make_table(kind, 3 * J + 1, 1 if kind == "mra" and sox == 1 else 0)
    return make_input(case_seed(name), soy, sox), J, ops, params


def hdr_input(h, w):
    """a smooth positive luminance with a bright spot, its minimum at zero (what hdr.c's shift by -low leaves)"""
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    lum = (0.02 + 0.5 * (x / w) * (y / h) + 40.0 * np.exp(-((x - 0.7 * w) ** 2 + (y - 0.3 * h) ** 2) / 30.0)).astype(F32)
    return (lum - lum.min()).astype(F32)
