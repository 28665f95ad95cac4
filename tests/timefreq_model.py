"""Model of libdwt's time-frequency planes (src/gabor.c), written from the reference's definition.

With x a line of N float32 samples and k a complex kernel of `size` taps around `center`,

    c(t) = (+0, +0);  for i = -min(t, center) .. min(N-1-t, size-center-1):
        c.re = fl32(c.re + fl32(x[t+i] * k[center+i].re));  c.im = fl32(c.im + fl32(x[t+i] * -k[center+i].im))

(dwt_util_cdot1_s: the conjugate product of a real sample, product and sum rounded separately, taps ascending); the
magnitude is fl32(sqrt(re*re + im*im)) evaluated in float64 -- both squares are exact there -- with hypot's rule for an
infinite part; bin y of a bank writes plane row bins-1-y.

* `cdots`, `magnitude`, `planes` -- the numpy float32 restatement;
* `phase_derivative`, `ridges1`, `ridges2` -- the plane operators, float32 operation by operation;
* `ridges3` -- detect_ridges3_s with the angle, its cosine and sine in float64 rounded once, as the device takes them;
* `ridges3_margin` -- how close the float64 cosine / sine of a point's gradient angle comes to +-1/2 (detect_ridges3_s);
* `CASES` -- what tests/golden/timefreq.npz holds, written by scripts/gen_timefreq_golden.py from the reference itself."""
import os

import numpy as np

from swt_model import make_input, same  # noqa: F401  (the seeded rows and the bitwise comparison of the SWT tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "timefreq.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "timefreq_manifest.json")

F32 = np.float32
PI = F32(np.pi)
TWO_PI = F32(F32(2) * PI)


def cdots(x, size, center, taps):
    """c(t) for every t of one line against one kernel (taps: complex64) -> (re, im) float32 arrays"""
    x = np.asarray(x, F32)
    n = len(x)
    t = np.arange(n)
    re, im = np.zeros(n, F32), np.zeros(n, F32)
    kr, ki = np.real(taps).astype(F32), (-np.imag(taps)).astype(F32)
    with np.errstate(all="ignore"):
        for j in range(size):
            idx = t - center + j
            ok = (idx >= 0) & (idx < n)
            s = x[np.clip(idx, 0, n - 1)]
            re = np.where(ok, (re + (s * kr[j]).astype(F32)).astype(F32), re)
            im = np.where(ok, (im + (s * ki[j]).astype(F32)).astype(F32), im)
    return re, im


def magnitude(re, im):
    with np.errstate(all="ignore"):
        re64, im64 = np.asarray(re, np.float64), np.asarray(im, np.float64)
        m = np.sqrt(re64 * re64 + im64 * im64).astype(F32)
    return np.where(np.isinf(re) | np.isinf(im), F32(np.inf), m).astype(F32)


def planes(x, sizes, centers, taps):
    """(re, im, magnitude) planes of shape (bins, N): bin y in row bins-1-y"""
    bins = len(sizes)
    re, im = np.zeros((bins, len(x)), F32), np.zeros((bins, len(x)), F32)
    for y in range(bins):
        re[bins - 1 - y], im[bins - 1 - y] = cdots(x, int(sizes[y]), int(centers[y]), taps[y])
    return re, im, magnitude(re, im)


def phase_derivative(angle, limit):
    a = np.asarray(angle, F32)
    out = np.zeros(a.shape, F32)
    with np.errstate(all="ignore"):
        d = ((-a[..., :-1]) + a[..., 1:]).astype(F32)
        for _ in range(64):
            hi = d > F32(limit)
            if not hi.any():
                break
            d = np.where(hi, (d - TWO_PI).astype(F32), d)
        for _ in range(64):
            lo = d < -F32(limit)
            if not lo.any():
                break
            d = np.where(lo, (d + TWO_PI).astype(F32), d)
    out[..., 1:] = d
    return out


def ridges1(mag, threshold):
    m = np.asarray(mag, F32)
    out = np.zeros(m.shape, F32)
    if m.shape[-1] < 3:
        return out
    with np.errstate(all="ignore"):
        m0, m1, m2 = m[..., :-2], m[..., 1:-1], m[..., 2:]
        f = ((F32(-1) * (m0 - m1).astype(F32)).astype(F32) * (m1 - m2).astype(F32)).astype(F32)
        v = ((m1 / F32(2)).astype(F32) / PI).astype(F32)
        out[..., 1:-1] = np.where((f > 0) & (m1 > F32(threshold)), v, F32(0))
    return out


def ridges2(freq, threshold):
    a = np.asarray(freq, F32)
    out = np.zeros(a.shape, F32)
    if a.shape[-1] < 3:
        return out
    with np.errstate(all="ignore"):
        m = a[..., 1:-1]
        v = ((np.abs(m) / F32(2)).astype(F32) / PI).astype(F32)
        out[..., 1:-1] = np.where((m < 0) & (np.abs(m) > F32(threshold)), v, F32(0))
    return out


def ridges3_margin(mag):
    """the smallest distance of |cos| or |sin| of an interior point's gradient angle (float64, of the float32 central
    differences) from 1/2; inf where the plane has no interior or no point with a number for an angle"""
    m = np.asarray(mag, F32)
    if m.shape[0] < 3 or m.shape[1] < 3:
        return np.inf
    with np.errstate(all="ignore"):
        dx = ((m[1:-1, 2:] - m[1:-1, :-2]).astype(F32) / F32(2)).astype(F32)
        dy = ((m[2:, 1:-1] - m[:-2, 1:-1]).astype(F32) / F32(2)).astype(F32)
        ang = np.arctan2(dy.astype(np.float64), dx.astype(np.float64))
        d = np.minimum(np.abs(np.abs(np.cos(ang)) - 0.5), np.abs(np.abs(np.sin(ang)) - 0.5))
    d = d[~np.isnan(d)]
    return float(d.min()) if d.size else np.inf


def ridges3(mag, threshold):
    """detect_ridges3_s the way the device evaluates it (libdwt_amd/csrc/dwt_timefreq.hip: grad_max): the gradient angle,
    its cosine and its sine each taken in float64 and rounded to float32 once.  The reference's float libm gives the same
    plane wherever no cosine or sine comes within `ridges3_margin` of -+1/2 (tests/test_grid_limits_model.py holds this
    function to the fixtures)."""
    m = np.asarray(mag, F32)
    out = np.zeros(m.shape, F32)
    if m.shape[0] < 3 or m.shape[1] < 3:
        return out
    with np.errstate(all="ignore"):
        m1 = m[1:-1, 1:-1]
        dx = ((m[1:-1, 2:] - m[1:-1, :-2]).astype(F32) / F32(2)).astype(F32)
        dy = ((m[2:, 1:-1] - m[:-2, 1:-1]).astype(F32) / F32(2)).astype(F32)
        ang = np.arctan2(dy.astype(np.float64), dx.astype(np.float64)).astype(F32).astype(np.float64)
        dir_x, dir_y = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
        nx = np.where(dir_x < F32(-0.5), -1, np.where(dir_x > F32(0.5), 1, 0))
        ny = np.where(dir_y < F32(-0.5), -1, np.where(dir_y > F32(0.5), 1, 0))
        yy, xx = np.mgrid[1:m.shape[0] - 1, 1:m.shape[1] - 1]
        keep = (m1 >= m[yy + ny, xx + nx]) & (m1 > F32(threshold))
        out[1:-1, 1:-1] = np.where(keep, ((m1 / F32(2)).astype(F32) / PI).astype(F32), F32(0))
    return out


def ulps(got, exact64):
    """|got - exact| in units of the float32 spacing at exact (NaN where either is NaN)"""
    with np.errstate(all="ignore"):
        e = np.asarray(exact64, np.float64)
        sp = np.spacing(np.maximum(np.abs(e).astype(F32), np.finfo(F32).tiny)).astype(np.float64)
        return np.abs(np.asarray(got, np.float64) - e) / sp


SIGMA_TF, FREQ_TF = 40.0, float(F32(0.999) * PI)  # examples/spectra-tf
SIGMA_EX, FREQ_EX = 10.0, float(F32(0.75) * PI)  # examples/time-freq (its STFT: sigma 20)
LIMIT = float(PI)

# (seed, kind, input, n, bins, sigma, freq): every N of {1, 2, 7, 64, 333, 1024}, every bins of {1, 5, 16, 64}, the three
# kinds, kernels longer than the signal (sigma 40: 321 taps; the S transform's low bins), the settings of the two example
# programs, and two rows of the whole float range
CASES = [
    (4101, "ft", "normal", 1, 1, SIGMA_TF, 0.0),
    (4102, "wt", "normal", 2, 5, 1.0, FREQ_TF),
    (4103, "st", "normal", 7, 5, 0.0, 0.0),
    (4104, "ft", "normal", 64, 16, SIGMA_TF, 0.0),
    (4105, "wt", "normal", 64, 64, 1.0, FREQ_TF),
    (4106, "st", "normal", 333, 16, 0.0, 0.0),
    (4107, "ft", "small_ints", 333, 5, 20.0, 0.0),
    (4108, "wt", "normal", 1024, 5, SIGMA_EX, FREQ_EX),
    (4109, "st", "small_ints", 1024, 1, 0.0, 0.0),
    (4110, "ft", "normal", 1024, 5, SIGMA_TF, 0.0),
    (4111, "st", "float_range", 64, 5, 0.0, 0.0),
    (4112, "ft", "float_range", 333, 1, SIGMA_EX, 0.0),
    (4113, "wt", "float_range", 64, 16, 1.0, FREQ_TF),
]
KIND_ID = {"ft": 0, "wt": 1, "st": 2}
