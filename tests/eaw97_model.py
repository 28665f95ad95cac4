"""A numpy restatement of libdwt's edge-avoiding CDF 9/7 wavelet ("WCDF 9/7"), written from the reference's semantics
(src/eaw-experimental.c:56-186 forward line, 188-298 inverse line, 300-482 drivers; constants src/inline.h:310-315).

float32 numpy arithmetic rounds every operation once, like the reference's C without contraction; one numpy operation
stands for each of the reference's.  |d|^alpha is exact for alpha 1 and 0; any other alpha is computed in double and
rounded once to float (`mode2`: what the GPU kernels do; glibc's powf differs from it by at most 1 ulp).

The fixtures of tests/golden/eaw97.npz (scripts/gen_eaw97_golden.py, from the compiled reference) pin it."""
import json
import os

import numpy as np

from eaw_model import ceil_div_pow2, levels, same_weights, written  # noqa: F401  (shared with the 5/3 model)

F = np.float32
EPS = F(1.0e-5)
TWO = F(2)
P1, U1, P2, U2 = F(1.58613434342059), F(-0.0529801185729), F(-0.8829110755309), F(0.4435068520439)
S1 = F(1.1496043988602)
S2 = F(1 / 1.1496043988602)  # the double quotient rounded to float (src/inline.h:315)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eaw97.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "eaw97_manifest.json")


def mode2(d, alpha):
    """|d|^alpha of the kernels' mode 2: pow in float64, rounded once to float32."""
    with np.errstate(all="ignore"):
        return np.power(d.astype(np.float64), float(alpha)).astype(F)


def weights(a, b, alpha):
    """dwt_eaw_w (src/eaw-experimental.c:56)."""
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
        p = np.ones_like(d) if alpha == 0 else d if alpha == 1 else mode2(d, alpha)
        return F(1) / (p + EPS)


def _lift(t, W, c, op, parity):
    """One phase in place: t[i] = op(t[i], (wL*t[l] + wR*t[r]) / (wL+wR) * (2.f*c)) on the samples of `parity`, in the
    reference's order (inner odd samples, the last sample, sample 0, inner even samples -- each phase only reads the
    other parity, so the order inside a phase does not matter)."""
    N = t.shape[1]
    k = TWO * c
    with np.errstate(all="ignore"):
        if parity == 1:
            i = np.arange(1, N - 2 + (N & 1), 2)
        else:
            i = np.arange(2, N - (N & 1), 2)
        wl, wr = W[:, i - 1], W[:, i]
        t[:, i] = op(t[:, i], (wl * t[:, i - 1] + wr * t[:, i + 1]) / (wl + wr) * k)
        if (N - 1) % 2 == parity:  # the last sample: an update when N is odd, a predict when N is even
            e = W[:, N - 2]
            t[:, N - 1] = op(t[:, N - 1], (e * t[:, N - 2] + e * t[:, N - 2]) / (e + e) * k)
        if parity == 0:
            w0 = W[:, 0]
            t[:, 0] = op(t[:, 0], (w0 * t[:, 1] + w0 * t[:, 1]) / (w0 + w0) * k)


def fwd_lines(X, alpha):
    """dwt_eaw97_f_ex_stride_s over the rows of X (lines x N): (result in sample order, weights lines x N; NaN where
    the reference writes nothing)."""
    X = np.asarray(X, dtype=F)
    L, N = X.shape
    w = np.full((L, N), np.nan, dtype=F)
    if N < 2:
        return X * S1, w
    W = weights(X[:, :-1], X[:, 1:], alpha)
    t = X.copy()
    m, p = np.subtract, np.add
    _lift(t, W, P1, m, 1)
    _lift(t, W, U1, p, 0)
    _lift(t, W, P2, m, 1)
    _lift(t, W, U2, p, 0)
    with np.errstate(all="ignore"):
        t[:, 0::2] *= S1
        t[:, 1::2] *= S2
    w[:, :-1] = W
    w[:, -1] = 0
    return t, w


def inv_lines(T, W):
    """dwt_eaw97_i_ex_stride_s: T (lines x N) in sample order, W the forward's weights of these lines."""
    t = np.array(T, dtype=F)
    L, N = t.shape
    if N < 2:
        return t * S2
    W = np.asarray(W, dtype=F)
    with np.errstate(all="ignore"):
        t[:, 0::2] *= S2
        t[:, 1::2] *= S1
    m, p = np.subtract, np.add
    _lift(t, W, U2, m, 0)
    _lift(t, W, P2, p, 1)
    _lift(t, W, U1, m, 0)
    _lift(t, W, P1, p, 1)
    return t


def mallat_fwd(img, size_i=None, j_max=-1, decompose_one=0, zero_padding=0, alpha=1.0):
    """dwt_eaw97_2f_s on img (soy x sox, the outer frame), in place.  Returns (j, wH, wV); wV[k] is (columns, rows)."""
    soy, sox = img.shape
    siy, six = size_i or (soy, sox)
    J = levels(False, sox, soy, j_max, decompose_one)
    wH, wV = [], []
    for j in range(J):
        Wo, Ho, Wd, Hd = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j), ceil_div_pow2(sox, j + 1), ceil_div_pow2(soy, j + 1)
        Wi, Hi = ceil_div_pow2(six, j), ceil_div_pow2(siy, j)
        out, w = fwd_lines(img[:Ho, :Wi], alpha)
        img[:Ho, :(Wi + 1) // 2] = out[:, 0::2]
        img[:Ho, Wd:Wd + Wi // 2] = out[:, 1::2]
        wH.append(w)
        out, w = fwd_lines(img[:Hi, :Wo].T, alpha)
        img[:(Hi + 1) // 2, :Wo] = out[:, 0::2].T
        img[Hd:Hd + Hi // 2, :Wo] = out[:, 1::2].T
        wV.append(w)
        if zero_padding:
            img[:Ho, (Wi + 1) // 2:Wd] = 0
            img[:Ho, Wd + Wi // 2:Wo] = 0
            img[(Hi + 1) // 2:Hd, :Wo] = 0
            img[Hd + Hi // 2:Ho, :Wo] = 0
    return J, wH, wV


def mallat_inv(img, wH, wV, size_i=None, j_max=-1, decompose_one=0, zero_padding=0):
    """dwt_eaw97_2i_s on img, in place."""
    soy, sox = img.shape
    siy, six = size_i or (soy, sox)
    for j in range(levels(True, sox, soy, j_max, decompose_one), 0, -1):
        Ws, Hs, Wo, Ho = ceil_div_pow2(sox, j), ceil_div_pow2(soy, j), ceil_div_pow2(sox, j - 1), ceil_div_pow2(soy, j - 1)
        Wi, Hi = ceil_div_pow2(six, j - 1), ceil_div_pow2(siy, j - 1)
        T = np.empty((Wo, Hi), dtype=F)
        T[:, 0::2] = img[:(Hi + 1) // 2, :Wo].T
        T[:, 1::2] = img[Hs:Hs + Hi // 2, :Wo].T
        img[:Hi, :Wo] = inv_lines(T, wV[j - 1]).T
        T = np.empty((Ho, Wi), dtype=F)
        T[:, 0::2] = img[:Ho, :(Wi + 1) // 2]
        T[:, 1::2] = img[:Ho, Ws:Ws + Wi // 2]
        img[:Ho, :Wi] = inv_lines(T, wH[j - 1])
        if zero_padding:
            img[:Ho, Wi:Wo] = 0
            img[Hi:Ho, :Wo] = 0
    return j_max


# ---- the fixture cases (scripts/gen_eaw97_golden.py writes them, tests/test_eaw97.py and test_hip_eaw97.py read them) ----
# (shape, size_i or None, j_max, decompose_one, zero_padding, alpha, input kind)
CASES = []
for _shape in [(1, 1), (1, 37), (37, 1), (2, 2), (2, 3), (3, 5), (4, 5), (9, 14)]:
    for _j, _d1 in [(-1, 0), (-1, 1), (0, 0), (1, 0), (3, 1), (40, 0)]:
        CASES.append((_shape, None, _j, _d1, 0, 1.0, "uniform"))
for _shape in [(37, 100), (61, 67)]:
    CASES.append((_shape, None, -1, 0, 0, 1.0, "uniform"))
CASES.append(((70, 75), None, 2, 0, 0, 1.0, "uniform"))
for _shape in [(3, 5), (37, 100)]:
    CASES.append((_shape, None, -1, 0, 0, 0.0, "uniform"))
CASES.append(((37, 100), None, -1, 0, 0, 0.8, "uniform"))
CASES.append(((70, 75), None, 2, 0, 0, 0.8, "uniform"))
for _zp in (0, 1):
    CASES.append(((40, 50), (29, 37), 3, 0, _zp, 1.0, "uniform"))
CASES.append(((20, 23), None, 2, 0, 0, 1.0, "mixed"))


KINDS = ("uniform", "mixed")  # uniform in [-4, 4); conftest.full_range_floats(klass="mixed")


def load_golden():
    """The fixture as a list of dicts: img, out (coefficients), back (the reference's inverse of out), wH, wV, and the
    case's parameters."""
    z = np.load(GOLDEN)
    cases = []
    n = 0
    while "c%d_meta" % n in z:
        h, w, siy, six, j_max, d1, zp, kind, j = (int(v) for v in z["c%d_meta" % n])
        cases.append(dict(img=z["c%d_in" % n], out=z["c%d_out" % n], back=z["c%d_back" % n], size_i=None if siy < 0 else (siy, six),
                          j_max=j_max, d1=d1, zp=zp, j=j, kind=KINDS[kind], alpha=float(z["c%d_alpha" % n]),
                          wH=[z["c%d_wH%d" % (n, k)] for k in range(j)], wV=[z["c%d_wV%d" % (n, k)] for k in range(j)]))
        n += 1
    return cases


def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def alpha_deviation(cases):
    """Largest |model(mode2 weights) - reference| over the coefficients of the fixture's forward cases with an alpha
    other than 0 and 1, relative to the case's largest coefficient (the manifest's alpha_dev_model)."""
    worst = 0.0
    for c in cases:
        if c["alpha"] in (0.0, 1.0):
            continue
        a = c["img"].copy()
        mallat_fwd(a, size_i=c["size_i"], j_max=c["j_max"], decompose_one=c["d1"], zero_padding=c["zp"], alpha=c["alpha"])
        worst = max(worst, float(np.abs(a.astype(np.float64) - c["out"].astype(np.float64)).max() / np.abs(c["out"]).max()))
    return worst


def roundtrip_deviation(cases):
    """Largest |reference inverse(reference forward(x)) - x| / max|x| over the fixture's dense cases with finite-range
    input (the manifest's roundtrip_ref)."""
    worst = 0.0
    for c in cases:
        if c["size_i"] is not None or c["kind"] != "uniform" or c["j"] == 0:
            continue
        worst = max(worst, float(np.abs(c["back"].astype(np.float64) - c["img"].astype(np.float64)).max() / np.abs(c["img"]).max()))
    return worst
