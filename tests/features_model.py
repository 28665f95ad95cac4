"""Models of libdwt's per-subband feature statistics (dwt_util_wps_s, _maxidx_s, _mean_s, _med_s, _var_s, _stdev_s,
_skew_s, _kurt_s, _maxnorm_s, _lpnorm_s, _norm_s; src/libdwt.c:23086-23786), written from the reference's definition:

* `bands` -- the band geometry of dwt_util_subband for levels 1 .. j_max-1 (level j_max is not visited), HL, LH, HH,
  empty bands skipped;
* `seq32` -- the literal restatement: float32 terms added one by one in row-major order, finished in float32;
* `model64` -- per band and statistic the float64 sums (value64, sum |term|, n) the GPU suite's bounds are built on;
* `finish` -- the host finalisation (float32, libm's powf / sqrtf) of given sums;
* `RefFeatures` -- the same entries of the compiled reference (oracle/_ref/libdwt_ref.so) where it was built.

Run as a program it writes tests/golden/features.npz from the compiled reference."""
import ctypes as C
import ctypes.util
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdwt_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "features.npz")

NAMES = ("wps", "maxidx", "mean", "med", "var", "stdev", "skew", "kurt", "maxnorm", "lpnorm", "norm")
F32 = np.float32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.argtypes = [C.c_float, C.c_float]
_libm.powf.restype = C.c_float


def powf(a, b):
    return F32(_libm.powf(float(a), float(b)))


def ceil_div_pow2(x, j):
    return (x + (1 << j) - 1) >> j


def bands(sox, soy, six, siy, j_max):
    """[(x0, y0, w, h, j)] in the reference's order."""
    out = []
    for j in range(1, min(j_max, 31)):
        hx, hy = ceil_div_pow2(six, j - 1) // 2, ceil_div_pow2(siy, j - 1) // 2
        lx, ly = ceil_div_pow2(six, j), ceil_div_pow2(siy, j)
        ox, oy = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j)
        for b in ((ox, 0, hx, ly, j), (0, oy, lx, hy, j), (ox, oy, hx, hy, j)):
            if b[2] and b[3]:
                out.append(b)
    return out


def count_subbands(sox, soy, six, siy, j_max):
    return len(bands(sox, soy, six, siy, j_max))


def band_values(img, b):
    x0, y0, w, h, _ = b
    return np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w], dtype=F32).reshape(-1)


def _seqsum(terms):
    """float32 terms added one by one, from 0.0f"""
    return F32(np.add.accumulate(np.concatenate(([F32(0)], np.asarray(terms, dtype=F32))), dtype=F32)[-1])


def _powf_each(a, e):
    return np.array([_libm.powf(float(v), float(e)) for v in a], dtype=F32)


def finish(name, sums, size, j, p):
    """The reference's arithmetic after the sums, in float32.  sums: dict of float32 S1 S2 Sp M2 M3 M4, maxnorm, maxidx, med."""
    n = F32(size)
    if name == "wps":
        return F32(sums["S2"] / F32(1 << j))
    if name == "mean":
        return F32(sums["S1"] / n)
    if name == "var":
        return F32(sums["M2"] / n)
    if name == "stdev":
        return np.sqrt(F32(sums["M2"] / n), dtype=F32)
    if name in ("skew", "kurt"):
        k = 3 if name == "skew" else 4
        stdev = np.sqrt(F32(sums["M2"] / n), dtype=F32)
        with np.errstate(all="ignore"):
            sm = F32(F32(sums["M%d" % k] / n) / powf(stdev, k))
        return sm if name == "skew" else F32(sm - F32(3))
    if name == "lpnorm" or name == "norm":
        pp = F32(2) if name == "norm" else F32(p)
        if math.isinf(pp):
            return F32(sums["maxnorm"])
        return powf(sums["S2"] if name == "norm" or pp == 2 else sums["Sp"], F32(1) / pp)
    return F32(sums[name])  # maxnorm, maxidx, med


def order_stats(v):
    a = np.abs(v)
    return {"maxnorm": F32(a.max()), "maxidx": F32(int(np.argmax(a))), "med": F32(np.sort(v, kind="stable")[len(v) // 2])}


def seq32_band(v, j, p):
    """Every statistic of one band as the reference computes it."""
    s = order_stats(v)
    s["S1"] = _seqsum(v)
    s["S2"] = _seqsum(v * v)
    mean = F32(s["S1"] / F32(len(v)))
    d = (v - mean).astype(F32)
    for k in (2, 3, 4):
        s["M%d" % k] = _seqsum(_powf_each(d, k))
    out = {}
    for name in NAMES:
        if name == "wps":
            out[name] = finish("wps", s, len(v), j, p)
        elif name == "lpnorm":
            if math.isinf(p):
                out[name] = s["maxnorm"]
            else:
                out[name] = powf(_seqsum(_powf_each(np.abs(v), p)), F32(1) / F32(p))
        elif name == "norm":
            out[name] = powf(_seqsum(_powf_each(np.abs(v), 2)), F32(1) / F32(2))
        else:
            out[name] = finish(name, s, len(v), j, p)
    return out


def seq32(img, sox, soy, six, siy, j_max, p):
    """{name: float32 vector} over the bands of a frame."""
    bs = bands(sox, soy, six, siy, j_max)
    per = [seq32_band(band_values(img, b), b[4], p) for b in bs]
    return {n: np.array([q[n] for q in per], dtype=F32) for n in NAMES}


def model64_band(v, p, mean=None):
    """The float64 sums of one band: {sum name: (value64, sum |term|, n)}; the terms are formed as the contract says:
    x*x and (x - mean)^2 exact, cubes and fourth powers rounded once, x - mean a float32 subtraction of the float32 mean,
    |x|^p (p other than 1, 2) pow in double rounded to float32.  `mean`: the float32 mean the central sums are taken about
    (default: the one of this model's own sum)."""
    x = v.astype(np.float64)
    out = {}

    def put(name, t):
        out[name] = (math.fsum(t), math.fsum(np.abs(t)), len(t))

    put("S1", x)
    put("S2", x * x)
    if p == 1:
        put("Sp", np.abs(x))
    elif p == 2 or math.isinf(p):
        put("Sp", x * x)
    else:
        put("Sp", np.power(np.abs(x), np.float64(F32(p))).astype(F32).astype(np.float64))
    mean = F32(F32(out["S1"][0]) / F32(len(v))) if mean is None else F32(mean)
    d = (v - mean).astype(F32).astype(np.float64)
    d2 = d * d
    put("M2", d2)
    put("M3", d2 * d)
    put("M4", d2 * d2)
    return out


class RefFeatures:
    """ctypes binding of the compiled reference's feature entries."""

    def __init__(self):
        self.lib = C.CDLL(REF_SO)
        I, P, F = C.c_int, C.c_void_p, C.c_float
        for n in NAMES:
            f = getattr(self.lib, "dwt_util_%s_s" % n)
            f.argtypes = [P, I, I, I, I, I, I, I, P] + ([F] if n == "lpnorm" else [])
            f.restype = None
        self.lib.dwt_util_count_subbands_s.argtypes = [P, I, I, I, I, I, I, I]
        self.lib.dwt_util_count_subbands_s.restype = I
        self.lib.dwt_util_abs_s.argtypes = [P, I, I, I, I]
        self.lib.dwt_util_abs_s.restype = None

    @staticmethod
    def available():
        return os.path.exists(REF_SO)

    def count(self, img, sox, soy, six, siy, j_max):
        return self.lib.dwt_util_count_subbands_s(img.ctypes.data, img.strides[0], 4, sox, soy, six, siy, j_max)

    def features(self, img, sox, soy, six, siy, j_max, p):
        img = np.ascontiguousarray(img, dtype=F32)
        n = self.count(img, sox, soy, six, siy, j_max)
        out = {}
        for name in NAMES:
            fv = np.zeros(max(n, 1), dtype=F32)
            args = [img.ctypes.data, img.strides[0], 4, sox, soy, six, siy, j_max, fv.ctypes.data]
            getattr(self.lib, "dwt_util_%s_s" % name)(*(args + ([float(p)] if name == "lpnorm" else [])))
            out[name] = fv[:n]
        return out


# ---- seeded inputs -----------------------------------------------------------------------------------------------------
# (seed, kind, sox, soy, six, siy, j_max, p)
CASES = []
for _i, (_w, _h, _j) in enumerate([(64, 1, 7), (100, 1, 5), (37, 1, 4), (1, 9, 3), (16, 16, 4), (33, 17, 4), (40, 24, 6), (8, 8, 1),
                                   (8, 8, 0), (5, 3, 5), (64, 48, 3)]):
    for _k, _p in (("normal", 2.0), ("uniform", 1.0), ("small_ints", 3.0), ("normal", 1.5), ("uniform", float("inf"))):
        CASES.append((1000 + 10 * _i + len(CASES) % 7, _k, _w, _h, _w, _h, _j, _p))
CASES += [(2001, "normal", 48, 40, 37, 29, 4, 2.0), (2002, "uniform", 64, 1, 50, 1, 6, 1.0), (2003, "small_ints", 32, 32, 17, 32, 5, 2.5)]


def make_input(seed, kind, sox, soy):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        a = rng.standard_normal((soy, sox)).astype(F32)
    elif kind == "uniform":
        a = rng.uniform(-1, 1, (soy, sox)).astype(F32)
    else:  # ties and both zeros
        a = rng.integers(-3, 4, (soy, sox)).astype(F32)
        a[rng.random((soy, sox)) < 0.1] = F32(-0.0)
    return a


def main():
    ref = RefFeatures()
    out = {"cases": np.array([(s, k, a, b, c, d, j, p) for (s, k, a, b, c, d, j, p) in CASES],
                             dtype=[("seed", "i4"), ("kind", "U12"), ("sox", "i4"), ("soy", "i4"), ("six", "i4"), ("siy", "i4"),
                                    ("j_max", "i4"), ("p", "f4")])}
    for i, (seed, kind, sox, soy, six, siy, j_max, p) in enumerate(CASES):
        img = make_input(seed, kind, sox, soy)
        f = ref.features(img, sox, soy, six, siy, j_max, p)
        out["count_%d" % i] = np.int32(ref.count(img, sox, soy, six, siy, j_max))
        for n in NAMES:
            out["%s_%d" % (n, i)] = f[n]
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
