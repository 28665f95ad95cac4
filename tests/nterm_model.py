"""Model of the N-term approximation: the non-linear branch of the reference's
examples/displ-vectors/vectors.c (:254-297) restated in numpy float32.

A group is C = 1 .. 4 frames, the transforms of the channels of one image.  Per position the magnitude is fabsf(c0) for
one channel and sqrtf(c0*c0 + c1*c1 [+ c2*c2 [+ c3*c3]]) otherwise, every product and sum rounded to float32 on its own,
summed left to right (numpy's float32 sqrt is correctly rounded, as libm's sqrtf is).  With M positions in scope and
n = keep (n = M where keep < 1 or keep > M), thr is element n-1 of the scope's magnitudes in descending order; every
position in scope with magnitude < thr gets +0 in every channel, ties at thr are kept.

* `magnitudes`, `scope_mask`, `threshold`, `keep_largest` -- the model; the select runs on the uint32 image of the
  magnitudes (they are never negative and never -0, so unsigned order is float order);
* `literal` -- the same as the reference writes it: a full descending sort, index n-1, strict <;
* `make_input`, `flow_fields` -- seeded groups; the flow fields use +, -, * and / of float64 alone, so that every
  machine builds the same bits;
* `CASES` -- what tests/golden/nterm.npz holds, written by scripts/gen_nterm_golden.py."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nterm.npz")
MANIFEST = os.path.join(ROOT, "tests", "golden", "nterm_manifest.json")

F32 = np.float32
FRAME, DETAILS = 0, 1  # enum dwt_hip_nterm_scope


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ceil_log2(x):
    n = 0
    while n < 31 and (1 << n) < x:
        n += 1
    return n


def band_levels(size_x, size_y, j_max=-1):
    """dwt_hip_band_levels"""
    lo, hi = min(size_x, size_y), max(size_x, size_y)
    if j_max < 0:
        return ceil_log2(hi if lo <= 1 else lo)
    return min(j_max, ceil_log2(hi))


def magnitudes(planes):
    """planes: (C, h, w) float32 -> (h, w) float32"""
    p = np.asarray(planes, F32)
    if p.shape[0] == 1:
        return np.abs(p[0])
    with np.errstate(all="ignore"):
        s = ((p[0] * p[0]).astype(F32) + (p[1] * p[1]).astype(F32)).astype(F32)
        for c in range(2, p.shape[0]):
            s = (s + (p[c] * p[c]).astype(F32)).astype(F32)
        return np.sqrt(s).astype(F32)


def scope_mask(size_y, size_x, scope=FRAME, j_max=-1):
    m = np.ones((size_y, size_x), bool)
    if scope == DETAILS:
        J = band_levels(size_x, size_y, j_max)
        m[:-(-size_y // (1 << J)), :-(-size_x // (1 << J))] = False
    return m


def threshold(mag, keep):
    """(thr, kept) over the magnitudes in scope (1-D, NaN-free); (0, 0) for an empty scope"""
    M = mag.size
    if M == 0:
        return F32(0), 0
    n = M if keep < 1 or keep > M else keep
    k = bits(mag)
    t = np.partition(k, M - n)[M - n]
    return np.array([t], np.uint32).view(F32)[0], int((k >= t).sum())


def keep_largest(planes, keep, scope=FRAME, j_max=-1):
    """-> (planes after the call, thr, kept)"""
    p = np.array(planes, F32)
    mag, m = magnitudes(p), scope_mask(p.shape[1], p.shape[2], scope, j_max)
    thr, kept = threshold(mag[m], keep)
    p[:, m & (mag < thr)] = F32(0)
    return p, thr, kept


def literal(planes, keep, scope=FRAME, j_max=-1):
    """vectors.c:273-297 word for word: the array, the descending sort, array[N-1], the strict comparison"""
    p = np.array(planes, F32)
    mag, m = magnitudes(p), scope_mask(p.shape[1], p.shape[2], scope, j_max)
    array = sorted((float(v) for v in mag[m]), reverse=True)
    if not array:
        return p, F32(0), 0
    N = keep
    if N < 1 or N > len(array):
        N = len(array)
    thr = F32(array[N - 1])
    kept = 0
    for y in range(p.shape[1]):
        for x in range(p.shape[2]):
            if not m[y, x]:
                continue
            if mag[y, x] < thr:
                p[:, y, x] = F32(0)
            else:
                kept += 1
    return p, thr, kept


KINDS = ("normal", "float_range", "ties", "underflow")


def make_input(seed, kind, channels, size_y, size_x):
    """one seeded NaN-free group (channels, size_y, size_x)"""
    rng = np.random.default_rng(seed)
    shape = (channels, size_y, size_x)
    if kind == "normal":
        return rng.standard_normal(shape).astype(F32)
    if kind == "float_range":  # every finite float, then a few infinities
        b = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
        b[(b & 0x7f800000) == 0x7f800000] &= np.uint32(0xbf7fffff)
        a = b.view(F32).copy()
        r = rng.random(shape)
        a[r < 0.01] = F32(np.inf)
        a[(r >= 0.01) & (r < 0.02)] = F32(-np.inf)
        return a
    if kind == "ties":
        return rng.integers(-3, 4, shape).astype(F32)
    assert kind == "underflow"  # squares that are subnormal or vanish, subnormal coefficients, signed zeros
    a = (rng.standard_normal(shape) * 1e-21).astype(F32)
    r = rng.random(shape)
    a[r < 0.2] = (rng.standard_normal(shape) * 1e-40).astype(F32)[r < 0.2]
    a[(r >= 0.2) & (r < 0.25)] = F32(-0.0)
    a[(r >= 0.25) & (r < 0.3)] = F32(0.0)
    return a


def flow_fields(size_y, size_x):
    """two smooth displacement fields (2, size_y, size_x): a rotation about a point off the centre with a shear, in
    pixels; float64 +, -, *, / alone, rounded to float32 once"""
    v, u = np.meshgrid(np.arange(size_y, dtype=np.float64) / size_y, np.arange(size_x, dtype=np.float64) / size_x, indexing="ij")
    a, b = u - 0.4, v - 0.55
    r2 = a * a + b * b
    dx = -6.0 * b / (1.0 + 4.0 * r2) + 1.5 * u * v
    dy = 6.0 * a / (1.0 + 4.0 * r2) - 2.0 * (u - 0.5) * (u - 0.5)
    return np.stack([dx, dy]).astype(F32)


def keeps_of(M):
    return [1, 2, M // 100, M // 10, M // 2, M - 1, M, 0, -1, M + 1]


# name -> (source, seed, wavelet, size_y, size_x): two-channel groups.  source "flow": the coefficient planes are the
# reference's forward transform (every level) of flow_fields and are stored; otherwise make_input(seed, source, 2, ..).
# For every case the fixture holds the magnitude plane and the thresholds and kept counts for keeps_of(size_y * size_x).
CASES = {
    "flow97": ("flow", 0, "cdf97", 96, 128),
    "flow53": ("flow", 0, "cdf53", 37, 53),
    "normal": ("normal", 5101, None, 37, 53),
    "range": ("float_range", 5102, None, 64, 48),
    "ties": ("ties", 5103, None, 40, 40),
    "underflow": ("underflow", 5104, None, 32, 33),
}


def case_planes(name, golden=None):
    """the two coefficient planes of a case: from the fixture for the flow cases, seeded otherwise"""
    source, seed, _, size_y, size_x = CASES[name]
    if source == "flow":
        return np.asarray((golden if golden is not None else np.load(GOLDEN))[name + ".coef"], F32)
    return make_input(seed, source, 2, size_y, size_x)
